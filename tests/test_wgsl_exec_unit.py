"""CPU: the WGSL-subset interpreter (oracle/wgsl_exec.py) on small programs written for this test - precedence, value semantics, scoping,
AbstractFloat constants, integer and float arithmetic rules, vectors.  Independent of the reference checkout: what the interpreter does
with the reference's shader is only as good as what it does here."""
import numpy as np
import pytest

from oracle import wgsl_exec as W

F = np.float32

SRC = """
struct Inner { v: vec3<f32>, k: i32, }
struct Outer { a: Inner, h: f32, }
const third = 1.0 / 3.0;
const PI: f32 = 3.1415926;
const twice = 2.0 * third;

fn precedence(x: f32, y: f32) -> f32 { return -x * 0.5 + y / 4.0 - x * y; }
fn abstract_once(x: f32) -> f32 { return x * (third - twice); }          // the parenthesis is ONE binary64 subtraction, rounded when it meets x
fn concrete_let() -> f32 { let t = 1.0 / 3.0; return t * 3.0; }          // let concretises: t is the f32 nearest to 1/3
fn int_div(a: i32, b: i32) -> i32 { return a / b; }
fn int_mix(a: i32) -> i32 { return (a - 1) / 2 * 2 + a % 3; }
fn frem(a: f32, b: f32) -> f32 { return a % b; }
fn vec_ops(a: vec3<f32>, b: vec3<f32>, s: f32) -> vec3<f32> { return (a + b * s - a.zxy) / 2.0; }
fn swz(a: vec4<f32>) -> vec3<f32> { return vec3<f32>(1.0, a.rg) + a.xzy; }
fn shadow(x: f32) -> f32 {
    var r = x;
    { let x = r * 2.0; r = x + 1.0; { let r2 = r; let x = r2 * r2; r = x; } }
    if r > 10.0 { let r = 0.5; return r + x; }
    return r;
}
fn copies() -> f32 {
    var o: Outer;
    o.a.v = vec3<f32>(1.0, 2.0, 3.0); o.a.k = 7; o.h = 0.25;
    var p = o;                       // a copy
    p.a.v = p.a.v * 2.0; p.h = 4.0;
    let q = p.a;                     // a copy of the inner struct
    p.a.k = 9;
    return o.a.v.y + p.a.v.y * 10.0 + f32(q.k) * 100.0 + f32(p.a.k) * 1000.0 + o.h;
}
fn touch(i: Inner) -> f32 { var j = i; j.k = j.k + 1; return f32(j.k); }
fn param_copy() -> f32 { var i: Inner; i.k = 4; let a = touch(i); return a * 10.0 + f32(i.k); }
fn arrays() -> i32 {
    var st: array<Inner, 4>;
    var n: u32 = 0;
    for (var i = 0; i < 4; i++) { var e: Inner; e.k = i * i; st[n] = e; n = n + 1; }
    var e2 = st[2]; e2.k = 100;
    var acc = 0;
    while (true) { if n == 0 { break; } n = n - 1; acc += st[n].k; }
    return acc + e2.k;
}
fn loops(n: i32) -> i32 { var s = 0; var i = 0; for (; i < n; i++) { if i == 5 { break; } s += i; } return s * 100 + i; }
fn mixes(a: f32, b: f32, t: f32) -> vec3<f32> { return vec3<f32>(mix(a, b, t), clamp(a, 0.0, 1.0), max(min(a, b), 0.25)); }
fn cmp(a: vec2<i32>, b: vec2<i32>) -> bool { return all(a == b) && !(a.x < b.y) || false; }
fn powers(x: f32) -> vec3<f32> { return vec3<f32>(pow(x, 2.0), pow(x, 5.0), pow(vec3<f32>(x), vec3<f32>(4.0)).z); }
fn distance_shadowed(a: vec3<f32>, b: vec3<f32>) -> f32 { let distance = a - b; return distance(a, b) + distance.x; }
"""


@pytest.fixture(scope="module")
def ns():
    return W.compile_source(SRC)


def v3(*c):
    return W.Vec(F(x) for x in c)


def test_precedence_and_unary_minus(ns):
    x, y = F(1.7), F(-2.3)
    assert ns["fn_precedence"](x, y) == ((-x) * F(0.5) + y / F(4.0)) - x * y


def test_abstract_float_constants_are_binary64_until_they_meet_an_f32(ns):
    assert isinstance(ns["C_third"], float) and ns["C_third"] == 1.0 / 3.0 and isinstance(ns["C_PI"], np.float32)
    x = F(3.0)
    assert ns["fn_abstract_once"](x) == x * F(1.0 / 3.0 - 2.0 * (1.0 / 3.0))
    assert ns["fn_concrete_let"]() == F(1.0 / 3.0) * F(3.0)


def test_integer_division_truncates_and_float_remainder_is_truncated(ns):
    assert [ns["fn_int_div"](a, b) for a, b in ((7, 2), (-7, 2), (7, -2), (-7, -2), (5, 0))] == [3, -3, -3, 3, 0]
    assert ns["fn_int_mix"](8) == (8 - 1) // 2 * 2 + 8 % 3
    assert ns["fn_frem"](F(5.5), F(1.0)) == F(0.5) and ns["fn_frem"](F(-5.5), F(1.0)) == F(-0.5) and ns["fn_frem"](F(7.25), F(2.0)) == F(1.25)


def test_vectors_swizzles_and_scalar_division(ns):
    a, b, s = v3(1, 2, 3), v3(0.5, -1, 4), F(0.3)
    r = ns["fn_vec_ops"](a, b, s)
    half = F(1.0) / F(2.0)                                                           # N2: vector / scalar = vector * (1 / scalar)
    want = [((a.c[i] + b.c[i] * s) - a.c[j]) * half for i, j in ((0, 2), (1, 0), (2, 1))]
    assert list(r.c) == want
    r = ns["fn_swz"](W.Vec(F(x) for x in (1, 2, 3, 4)))
    assert list(r.c) == [F(1) + F(1), F(1) + F(3), F(2) + F(2)]


def test_block_scoping_and_shadowing(ns):
    # r = x; inner: x' = 2r; r = x'+1; innermost: x'' = r*r; r = x''   ->  (2x+1)^2 ; > 10 -> 0.5 + the PARAMETER x
    assert ns["fn_shadow"](F(1.0)) == F(9.0)
    assert ns["fn_shadow"](F(2.0)) == F(0.5) + F(2.0)


def test_structs_arrays_and_parameters_are_values(ns):
    assert ns["fn_copies"]() == F(2.0) + F(4.0) * F(10.0) + F(7) * F(100.0) + F(9) * F(1000.0) + F(0.25)
    assert ns["fn_param_copy"]() == F(5.0) * F(10.0) + F(4.0)
    assert ns["fn_arrays"]() == (0 + 1 + 4 + 9) + 100


def test_loops_break_and_compound_assignment(ns):
    assert ns["fn_loops"](3) == (0 + 1 + 2) * 100 + 3
    assert ns["fn_loops"](9) == (0 + 1 + 2 + 3 + 4) * 100 + 5


def test_builtins_follow_the_literal_conventions(ns):
    a, b, t = F(1.5), F(-0.5), F(0.25)
    r = ns["fn_mixes"](a, b, t)
    assert list(r.c) == [a * (F(1.0) - t) + b * t, F(1.0), F(0.25)]
    x = F(1.1)
    r = ns["fn_powers"](x)
    assert list(r.c) == [x * x, ((x * x) * (x * x)) * x, (x * x) * (x * x)]
    assert ns["fn_cmp"](W.Vec((3, 1)), W.Vec((3, 1))) is True and ns["fn_cmp"](W.Vec((0, 1)), W.Vec((0, 1))) is False


def test_a_local_named_like_a_builtin_does_not_hide_the_call(ns):
    a, b = v3(1, 2, 2), v3(0, 0, 0)
    assert ns["fn_distance_shadowed"](a, b) == F(3.0) + F(1.0)       # `let distance` in hit_torus2d (ray.wgsl:682, 693)


def test_a_loop_that_cannot_end_is_left_after_a_repeated_state():
    ns = W.compile_source("""
fn stuck(h0: f32) -> f32 { var h = h0; var n = 0; while true { n += 1; let t = 0.9 * h; if t > h { break; } h = max(t, h); if n > 1000 { break; } } return f32(n); }
""".replace("n += 1;", ""))
    # without the counter the state (h) repeats at once: the interpreter leaves the loop instead of spinning (D1)
    assert ns["fn_stuck"](F(1.0)) == F(0.0)


def test_syntax_outside_the_subset_is_refused():
    with pytest.raises(SyntaxError):
        W.compile_source("fn f() -> f32 { var i = 0; loop { continue; } return 1.0; }")
    with pytest.raises(NameError):
        W.compile_source("fn f() -> f32 { return undefined_thing; }")


# ---- the constructs of the display-pass shaders (oracle/wgsl_exec_post.py runs them); WGSL written for these tests
POST_SRC = """
struct Knobs { gain: f32, count: i32, bias: f32, flags: u32, };
struct Small { ratio: f32 }
struct Corner { @location(0) tc: vec2<f32>, @builtin(position) at: vec4<f32>, }
struct Pair { @builtin(position) p: vec4<f32>, @location(0) q: vec2<f32>, }
struct Box { lo: vec2<f32>, hi: vec2<f32>, }

@group(0) @binding(0) var tex: texture_2d<f32>;
@group(0) @binding(1) var smp: sampler;
@group(0) @binding(2) var<uniform> knobs: Knobs;
@group(0) @binding(3) var<uniform> small: Small;

fn pick(k: i32) -> f32 {
    switch (k) {
        case 3:            { return 30.0; }
        default:           { return -1.0; }
        case 4, 5, 6:      { return 40.0; }
        case 9:            { return 90.0; }
    }
}
fn pick_last(k: i32) -> i32 { var r = 0; switch k { case 1, 2 { r = 10; } case 7, default { r = 70; } } return r + 1; }
fn pick_first(k: i32) -> i32 { switch k { default: { return 0; } case 2: { return 2; } } }

@vertex
fn vtri(@builtin(vertex_index) n: u32) -> Corner {          // the corner is picked by comparing the index; uv computed from it
    var c = vec2<f32>(-1.0, 1.0);
    if (n == 1u) { c.y = -3.0; }
    if (n == 2u) { c.x = 3.0; }
    var o: Corner;
    o.at = vec4<f32>(c, 0.0, 1.0);
    o.tc = vec2<f32>(0.5 * c.x + 0.5, 0.5 - 0.5 * c.y);
    return o;
}
@vertex
fn vpair(@builtin(vertex_index) n: u32) -> Pair {
    let x = select(-1.0, 3.0, n == 2u);
    let y = select(1.0, -3.0, n == 1u);
    return Pair(vec4<f32>(x, y, 0.0, 1.0), vec2<f32>((x + 1.0) / 2.0, (1.0 - y) / 2.0));
}
fn grow(b: Box, d: f32) -> Box { var r = b; r.lo.x = r.lo.x - d; r.hi.y = r.hi.y + d * 2.0; return r; }
@fragment
fn fs_main(at: Pair) -> @location(0) vec4<f32> { return vec4<f32>(at.p.xy * at.q, at.p.w, knobs.gain); }

fn comp_assign(a: vec2<f32>, s: f32) -> vec2<f32> {
    var v = a; var w = vec2<f32>(0.0, 0.0);
    v.y = v.y + s * 0.5;
    w.x = a.x;
    v.x += w.x;
    return v - w;
}
fn m9(v: vec3<f32>) -> vec3<f32> {
    let m = mat3x3(
        1.0, 2.0, 3.0,
        0.5, 0.25, 0.125,
        -1.0, 10.0, 0.1,
    );
    return m * v;
}
fn abstract_let(a: f32) -> vec2<f32> { let e = 0.0035; return vec2<f32>(a - e, a + e); }
fn bools(a: f32, b: f32) -> vec3<f32> {
    let lt = a < b;
    let d = (a < 0.0) != lt;
    let e = (b < 0.0) != lt;
    var r = vec3<f32>(0.0);
    if (d) { r.x = 1.0; }
    if (!e) { r.y = 1.0; }
    if (d != e) { r.z = 1.0; }
    return r;
}
fn selects(a: f32, b: f32, c: bool) -> vec4<f32> {
    let s = select(a, b, c);
    let v = select(vec2<f32>(a, a), vec2<f32>(b, b) * 2.0, c);
    let z = select(0.0, b, c);
    return vec4<f32>(s, v, z);
}
fn select_lanes(a: vec3<f32>, b: vec3<f32>) -> vec3<f32> { return select(a, b, a < b); }
fn for_break(n: i32, stop: i32) -> i32 {
    var seen = 0;
    for (var i: i32 = 0; i < n; i = i + 1) {
        seen = seen + 100;
        if (i == stop) { break; }
        seen = seen + 1;
    }
    return seen;
}
fn dims() -> vec2<f32> { return 1.0 / vec2<f32>(textureDimensions(tex)); }
fn plain(uv: vec2<f32>) -> vec4<f32> { return textureSample(tex, smp, uv); }
fn level(uv: vec2<f32>) -> vec4<f32> { return textureSampleLevel(tex, smp, uv, 0.0); }
fn level_off(uv: vec2<f32>) -> vec3<f32> { return textureSampleLevel(tex, smp, uv, 0.0, vec2<i32>(1, -1)).rgb; }
fn uniforms() -> vec4<f32> { return vec4<f32>(knobs.gain, f32(knobs.count), knobs.bias, small.ratio) * f32(knobs.flags); }
"""


@pytest.fixture(scope="module")
def post():
    from oracle import wgsl_exec_post as WP
    sh = WP.Shader("unit", POST_SRC)
    rng = np.random.default_rng(5)
    img = (rng.random((3, 5, 4)) * 4 - 1).astype(np.float16)                  # 5 wide, 3 high; binary16 texels, some negative
    sh.bind({0: WP.texture16(img), 2: np.array([1.5, 0, 0.25, 0], np.float32).tobytes()[:4] + (7).to_bytes(4, "little", signed=True)
             + np.float32(0.25).tobytes() + (3).to_bytes(4, "little"), 3: np.float32(0.7).tobytes()})
    return sh, img.astype(np.float32), WP


def test_switch_with_multi_value_cases_and_default_anywhere(post):
    ns = post[0].ns
    assert [ns["fn_pick"](k) for k in (3, 4, 5, 6, 9, 0, 7, -3)] == [F(30), F(40), F(40), F(40), F(90), F(-1), F(-1), F(-1)]
    assert [ns["fn_pick_last"](k) for k in (1, 2, 7, 5)] == [11, 11, 71, 71]
    assert [ns["fn_pick_first"](k) for k in (2, 3)] == [2, 0]
    with pytest.raises(SyntaxError):
        W.compile_source("fn f(k: i32) -> i32 { switch k { case 1: { return 1; } } return 0; }")           # no default
    with pytest.raises(SyntaxError):
        W.compile_source("fn f(k: i32) -> i32 { var r = 0; switch k { case 1: { break; } default: { r = 1; } } return r; }")


def test_entry_points_with_struct_io_builtins_and_value_constructors(post):
    sh = post[0]
    ns, meta = sh.ns, sh.meta
    assert meta[("fn", "vtri")] == [("vertex", [])] and meta[("fn", "fs_main")] == [("fragment", [])]
    assert meta[("param", "vtri", "n")] == [("builtin", ["vertex_index"])]
    assert meta[("field", "Corner", "at")] == [("builtin", ["position"])] and meta[("field", "Pair", "q")] == [("location", ["0"])]
    assert meta[("gvar", "knobs")] == [("group", ["0"]), ("binding", ["2"])]
    got = [(ns["fn_vtri"](i).tc.c, ns["fn_vtri"](i).at.c) for i in range(3)]
    assert got == [((F(0), F(0)), (F(-1), F(1), F(0), F(1))), ((F(0), F(2)), (F(-1), F(-3), F(0), F(1))), ((F(2), F(0)), (F(3), F(1), F(0), F(1)))]
    o = ns["fn_vpair"](2)                                                           # Pair(p, q): a struct value constructor
    assert o.q.c == (F(2), F(0)) and o.p.c == (F(3), F(1), F(0), F(1))
    # the fragment stage: position = pixel centre, the @location input interpolated there (rule R1)
    r = sh.fragment(2, 1, 5, 3)
    u, v = (F(2) + F(0.5)) / F(5), (F(1) + F(0.5)) / F(3)
    assert r.c == (F(2.5) * u, F(1.5) * v, F(1.0), F(1.5))


def test_vertex_stage_is_run_and_a_flipped_map_is_refused(post):
    WP = post[2]
    ok = POST_SRC.replace("fn vtri", "fn vs_main")
    assert WP.Shader("unit", ok).vertex_stage() == 3
    with pytest.raises(AssertionError, match="affine map"):
        WP.Shader("unit", ok.replace("0.5 - 0.5 * c.y", "0.5 + 0.5 * c.y")).vertex_stage()     # v = 0 on the BOTTOM row: not the rule's map
    ok2 = POST_SRC.replace("fn vpair", "fn vs_main")
    assert WP.Shader("unit", ok2).vertex_stage() == 3
    with pytest.raises(AssertionError, match="cover"):
        WP.Shader("unit", ok2.replace("select(-1.0, 3.0, n == 2u)", "select(-1.0, 1.0, n == 2u)")).vertex_stage()   # the corner (1, -1) is left bare


def test_component_assignment_through_a_swizzle(post):
    ns = post[0].ns
    a, s = W.Vec((F(0.3), F(0.7))), F(0.2)
    assert ns["fn_comp_assign"](a, s).c == ((a.c[0] + a.c[0]) - a.c[0], (a.c[1] + s * F(0.5)) - F(0.0))
    b = ns["S_Box"](W.Vec((F(1), F(2))), W.Vec((F(3), F(4))))                    # a component of a struct member; the argument stays as it was
    r = ns["fn_grow"](b, F(0.25))
    assert r.lo.c == (F(0.75), F(2)) and r.hi.c == (F(3), F(4.5)) and b.lo.c == (F(1), F(2)) and b.hi.c == (F(3), F(4))


def test_mat3x3_of_nine_scalars_is_column_major(post):
    v = v3(0.3, -2.0, 7.0)
    c0, c1, c2 = v3(1, 2, 3), v3(0.5, 0.25, 0.125), v3(-1, 10, 0.1)
    want = (c0 * v.c[0] + c1 * v.c[1]) + c2 * v.c[2]
    assert post[0].ns["fn_m9"](v).c == want.c


def test_an_abstract_let_is_rounded_once(post):
    a = F(0.3)
    assert post[0].ns["fn_abstract_let"](a).c == (a - F(0.0035), a + F(0.0035))


def test_bool_inequality_and_select(post):
    ns = post[0].ns
    assert ns["fn_bools"](F(-1), F(2)).c == (F(0), F(0), F(1))             # lt = T; d = (T != T) = F; e = (F != T) = T
    assert ns["fn_bools"](F(1), F(-2)).c == (F(0), F(0), F(1))             # lt = F; d = F; e = T
    assert ns["fn_bools"](F(-3), F(-2)).c == (F(0), F(1), F(0))            # lt = T; d = F; e = F
    assert ns["fn_bools"](F(2), F(1)).c == (F(0), F(1), F(0))
    a, b = F(1.25), F(-2.5)
    assert ns["fn_selects"](a, b, True).c == (b, b * F(2), b * F(2), b) and ns["fn_selects"](a, b, False).c == (a, a, a, F(0))
    assert ns["fn_select_lanes"](v3(1, 5, 3), v3(2, 4, 3)).c == (F(2), F(5), F(3))


def test_for_with_break_and_the_hit_counts(post):
    sh = post[0]
    ns = sh.ns
    sh.reset_counts()
    assert ns["fn_for_break"](4, 2) == 100 + 1 + 100 + 1 + 100            # i = 0, 1, then 2 breaks before the + 1
    assert ns["fn_for_break"](2, 9) == 202                                 # ends by its bound
    assert ns["fn_for_break"](0, 9) == 0
    hit, br, _ = sh.counts()
    sites = ns["__sites__"]
    loop = [i for i in sites["cond"]["for_break"] if br[(i, True)] == 5][0]
    inner = [i for i in sites["cond"]["for_break"] if i != loop][0]
    assert br[(loop, False)] == 2 and br[(inner, True)] == 1 and br[(inner, False)] == 4
    assert sorted(hit[i] for i in sites["stmt"]["for_break"]) == [1, 3, 3, 3, 4, 5, 5]     # break, var, for, return, + 1, + 100, if
    assert all(hit[i] == 0 for i in sites["stmt"]["pick"])                                  # never run: the key is simply absent
    sh.reset_counts()
    ns["fn_selects"](F(1), F(2), True)
    assert sorted(sh.counts()[2].values()) == [1, 1, 1] and all(k[1] is True for k in sh.counts()[2])


def test_float_textures_dimensions_and_samplers(post):
    sh, img, WP = post
    ns = sh.ns
    assert ns["fn_dims"]().c == (F(1.0) / F(5), F(1.0) / F(3))
    uv = W.Vec((F(0.61), F(0.4)))
    # textureSample: nearest when the source is larger than the target (min filter), bilinear when smaller (mag filter), the texel at 1:1
    sh.sampler.scale = 2.0
    assert ns["fn_plain"](uv).c == tuple(img[1, 3])                        # floor(0.61 * 5) = 3, floor(0.4 * 3) = 1
    sh.sampler.scale = 1.0
    assert ns["fn_plain"](uv).c == tuple(img[1, 3])
    # bilinear, written out: x = u * n - 0.5, then the offset
    def bil(ox, oy):
        x = F(0.61) * F(5) - F(0.5) + F(ox); y = F(0.4) * F(3) - F(0.5) + F(oy)
        x0, y0 = int(np.floor(x)), int(np.floor(y))
        tx, ty = x - np.floor(x), y - np.floor(y)
        cl = lambda i, n: min(max(i, 0), n - 1)                            # noqa: E731
        out = []
        for ch in range(4):
            a, b = img[cl(y0, 3), cl(x0, 5), ch], img[cl(y0, 3), cl(x0 + 1, 5), ch]
            c, d = img[cl(y0 + 1, 3), cl(x0, 5), ch], img[cl(y0 + 1, 3), cl(x0 + 1, 5), ch]
            out.append((a * (F(1) - tx) + b * tx) * (F(1) - ty) + (c * (F(1) - tx) + d * tx) * ty)
        return tuple(out)
    sh.sampler.scale = 0.5
    assert ns["fn_plain"](uv).c == bil(0, 0)
    sh.sampler.scale = 2.0                                                 # an explicit level 0 is bilinear whatever the pass's scale
    assert ns["fn_level"](uv).c == bil(0, 0)
    assert ns["fn_level_off"](uv).c == bil(1, -1)[:3]                      # y0 - 1 = -1: ClampToEdge
    assert ns["fn_level"](W.Vec((F(-0.3), F(1.7)))).c == tuple(img[2, 0])  # far outside: the corner texel


def test_uniform_structs_from_raw_bytes(post):
    sh = post[0]
    assert sh.ns["fn_uniforms"]().c == (F(1.5) * F(3), F(7) * F(3), F(0.25) * F(3), F(0.7) * F(3))
    with pytest.raises(AssertionError):
        sh.uniform("Knobs", b"\0" * 12)


def test_srgb_store_of_the_post_module_is_the_definition():
    from oracle import wgsl_exec_post as WP
    assert WP.srgb8(np.array([0.0, -1.0, 1.0, 7.0, 0.0031308, 0.5, 0.2140411])).tolist() == [0, 0, 255, 255, 10, 188, 127]
    assert WP.unorm8(np.array([-1.0, 0.25, 0.5 / 255 + 1e-9, 1.5 / 255, 2.5 / 255, 1.0, 3.0])).tolist() == [0, 64, 1, 2, 2, 255, 255]
    assert WP.bloom_sizes(32, 47) == [(16, 23), (8, 11), (4, 5), (2, 2), (1, 1), (2, 2), (4, 5), (8, 11), (16, 23), (32, 47)]
