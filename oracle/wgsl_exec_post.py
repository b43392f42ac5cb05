"""wgsl_exec_post.py - executes the REFERENCE'S OWN display-pass shader text.  TEST INFRASTRUCTURE ONLY; the shaders are read only where
/root/reference exists (the build container).

The display pass is everything behind the sky image: bloom_down.wgsl x5, bloom_up.wgsl x5, mix.wgsl, hdr.wgsl and
fxaa.wgsl, wired as src/renderer/mod.rs:209-324 wires them.  This module READS those five files at run time, has oracle/wgsl_exec.py parse
and translate them, and runs them as the render passes run them: `vs_main` on the vertices the pipeline draws, then `fs_main` once per
pixel of the target.  Nothing of the shaders is restated here: change a tap weight, a matrix entry, a `select` or a `case` in the text
and the images this module produces change with it.  The number of bloom passes and their scale factor are read from mod.rs, the quad's
corners from quad.rs, as data.

Arithmetic is the literal evaluation of wgsl_exec.py's header (N0-N6): one binary32 operation per operator in text order, AbstractFloat
constants in binary64 until they meet an f32, matrix * vector as (c0 * x + c1 * y) + c2 * z, dot as wgsl_exec sums it, division and sqrt
correctly rounded, min / max / clamp by compare-select.

What WGSL and wgpu leave to the implementation is THE PROJECT'S RULE (DESIGN.md §10 rules 2 and 3), stated here and nowhere inferred from
tests/post_ref.py or from the kernels:
  R1  rasterisation: the fragment of pixel (x, y) of a W' x H' target has position = (x + 0.5, y + 0.5, 0, 1) and every @location input
      interpolated at that point.  The vertex stage IS executed (vertex_stage below): its outputs must be the affine map
      uv = ((clip.x + 1) / 2, (1 - clip.y) / 2) on triangles that cover the viewport, i.e. uv (0, 0) at the top-left corner; the
      interpolated uv is then ((x + 0.5) / W', (y + 0.5) / H'), each one f32 addition and one correctly rounded f32 division.
  R2  samplers are ClampToEdge, mag Linear, min Nearest (bloom_pipline.rs:121-127 and the same lines of mix / hdr / fxaa_pipline.rs).
      `textureSample` takes its level of detail from the pass's scale: a source larger than the target (a down pass) is minified - a
      nearest fetch of texel floor(u * n), clamped; a source smaller than the target (an up pass) is magnified - bilinear; at 1:1 the
      sample is the texel the coordinate lies in (the texel itself for a fragment's own uv).  `textureSampleLevel(..., 0.0)` is bilinear.
  R3  bilinear (written here on its own): the texel coordinate is u * n - 0.5 (two f32 operations), an integer `offset` is added to it
      after the -0.5, i = floor, t = coordinate - i, the two indices clamp to [0, n - 1], and the four texels are combined as
      (a * (1 - tx) + b * tx) * (1 - ty) + (c * (1 - tx) + d * tx) * ty - along x first, one f32 operation per operator.
  R4  every pass target is Rgba16Float: the f32 result of `fs_main` is rounded to binary16, nearest even, after each pass.  The FXAA
      target is Rgba8UnormSrgb; its f32 result is kept, and the 8-bit image is encoded HERE from the definition evaluated in binary64:
      floor(255 * encode(clamp(v, 0, 1)) + 0.5) with encode(c) = 12.92 c below 0.0031308 and 1.055 c^(1/2.4) - 0.055 above - no threshold
      table.  Alpha is not encoded: rint(clamp(a, 0, 1) * 255) with the product in f32 (DESIGN §10 rule 6).  Which byte an alpha takes whose
      exact product lies within an f32 rounding of k + 0.5 is a driver's choice (as the rasteriser tie of rule 3 is) and is not pinned.
Non-finite input is outside the pin: compare-select `clamp` passes a NaN through where DESIGN §10.4 stores 0, so fixtures are finite.

Every statement that runs is counted (wgsl_exec.compile_source(count=True)): per shader a hit count per statement, per outcome of every
`if` / loop condition and per outcome of every scalar `select`, keyed by the token index of the statement in its file.
render_post(sky16, fxaa_bytes, mix_bytes) is the whole pass; tests/golden/make_golden_wgsl_post.py commits its images, tests/test_wgsl_post_pin.py
and tests/test_gpu_display_pin.py hold tests/post_ref.py and the kernels to them.
"""
from __future__ import annotations

import collections
import os
import re
import struct

import numpy as np

from . import wgsl_exec as W

F = np.float32
REF = "/root/reference/src/renderer"
STAGES = ("down", "up", "mix", "hdr", "fxaa")
FILES = {"down": "bloom_down.wgsl", "up": "bloom_up.wgsl", "mix": "mix.wgsl", "hdr": "hdr.wgsl", "fxaa": "fxaa.wgsl"}
FXAA_DEFAULT = struct.pack("<ffif", 0.0156, 0.063, 12, 0.75)       # what Renderer::render uploads every frame
MIX_DEFAULT = struct.pack("<f", 0.7)


def available():
    return all(os.path.exists(os.path.join(REF, "shaders", f)) for f in FILES.values())


def shader_text(stage):
    return open(os.path.join(REF, "shaders", FILES[stage])).read()


# ------------------------------------------------------------------------------------------------------------------ textures and samplers
class Sampler:
    """ClampToEdge, mag Linear, min Nearest (R2).  `scale` is set by the pass runner: source texels per target pixel, the larger axis."""

    def __init__(self):
        self.scale = 1.0


def texture16(img16):
    """A texture whose texels are a binary16 image (H x W x 4 float16, or its uint16 view)."""
    a = np.asarray(img16)
    if a.dtype == np.uint16:
        a = a.view(np.float16)
    assert a.dtype == np.float16 and a.ndim == 3 and a.shape[2] == 4
    return W.Texture(f32img=np.ascontiguousarray(a.astype(np.float32)))


def _vec4(row):
    return W.Vec((F(row[0]), F(row[1]), F(row[2]), F(row[3])))


def _fetch_nearest(t, u, v):
    w, h = t.size
    xi = int(np.floor(F(u) * F(w)))
    yi = int(np.floor(F(v) * F(h)))
    return _vec4(t.img[min(max(yi, 0), h - 1), min(max(xi, 0), w - 1)])


def _linear_axis(c, n, off):
    x = F(c) * F(n) - F(0.5)
    x = x + F(off)
    i = np.floor(x)
    t = x - i
    i = int(i)
    return min(max(i, 0), n - 1), min(max(i + 1, 0), n - 1), t


def _fetch_bilinear(t, u, v, ox=0, oy=0):
    w, h = t.size
    x0, x1, tx = _linear_axis(u, w, ox)
    y0, y1, ty = _linear_axis(v, h, oy)
    one = F(1.0)
    a, b, c, d = t.img[y0, x0], t.img[y0, x1], t.img[y1, x0], t.img[y1, x1]       # float32 rows: numpy rounds every elementwise operation
    top = a * (one - tx) + b * tx
    bot = c * (one - tx) + d * tx
    return _vec4(top * (one - ty) + bot * ty)


def bi_textureSample(t, s, uv):
    if s.scale < 1.0:
        return _fetch_bilinear(t, uv.c[0], uv.c[1])
    return _fetch_nearest(t, uv.c[0], uv.c[1])


def bi_textureSampleLevel(t, s, uv, lvl, off=None):
    assert float(lvl) == 0.0, "one mip level"
    ox, oy = (off.c[0], off.c[1]) if off is not None else (0, 0)
    return _fetch_bilinear(t, uv.c[0], uv.c[1], ox, oy)


# ------------------------------------------------------------------------------------------------------------------ one shader
class Shader:
    """One of the five files, translated with hit counting; sources[stage] replaces the file's text (mutation tests)."""

    def __init__(self, stage, text=None):
        self.stage = stage
        self.ns = W.compile_source(text if text is not None else shader_text(stage), name="<%s>" % stage, count=True)
        self.ns["bi_textureSample"] = bi_textureSample
        self.ns["bi_textureSampleLevel"] = bi_textureSampleLevel
        self.meta = self.ns["__meta__"]
        self.decls = self.ns["__decls__"]
        self.fn = {d[1]: d for d in self.decls if d[0] == "fn"}
        self.gvars = {d[1]: d[2] for d in self.decls if d[0] == "gvar"}
        self.sampler = Sampler()

    def _attr(self, key, name):
        for a, args in self.meta.get(key, ()):
            if a == name:
                return args
        return None

    def bind(self, resources):
        """resources: {@binding index: Texture | bytes of a uniform struct | None for the sampler}"""
        for name, ty in self.gvars.items():
            b = int(self._attr(("gvar", name), "binding")[0])
            if ty[0] == "sampler":
                self.ns["G_" + name] = self.sampler
            elif ty[0] == "texture_2d":
                self.ns["G_" + name] = resources[b]
            else:
                self.ns["G_" + name] = self.uniform(ty[0], resources[b])

    def uniform(self, struct_name, data):
        """a var<uniform> struct of 4-byte scalars from its raw bytes"""
        cls = self.ns["S_" + struct_name]
        data = bytes(data)
        assert len(data) == 4 * len(cls.FIELDS), "%s: %d bytes for %d fields" % (struct_name, len(data), len(cls.FIELDS))
        vals = []
        for i, (_, ty) in enumerate(cls.FIELDS):
            fmt = {"f32": "<f", "i32": "<i", "u32": "<I"}[ty[0]]
            vals.append(struct.unpack_from(fmt, data, 4 * i)[0])
        return cls(*vals)

    def _io_fields(self, struct_name):
        pos = loc = None
        for fname, _ in self.ns["S_" + struct_name].FIELDS:
            if self._attr(("field", struct_name, fname), "builtin") == ["position"]:
                pos = fname
            elif self._attr(("field", struct_name, fname), "location") == ["0"]:
                loc = fname
        assert pos is not None and loc is not None
        return pos, loc

    def vertex_stage(self, vertices=None):
        """Runs vs_main on the vertices the pipeline draws (vertex_index 0..2, or the given (position, tex_coords) list) and asserts R1's
        premise.  Returns the number of vertices run."""
        _, _, params, ret, _ = self.fn["vs_main"]
        assert self._attr(("fn", "vs_main"), "vertex") is not None
        pname, pty = params[0]
        outs = []
        if self._attr(("param", "vs_main", pname), "builtin") == ["vertex_index"]:
            assert vertices is None
            outs = [self.ns["fn_vs_main"](i) for i in range(3)]
        else:
            cls = self.ns["S_" + pty[0]]
            by_loc = {int(self._attr(("field", pty[0], f), "location")[0]): f for f, _ in cls.FIELDS}
            for p, uv in vertices:                                          # @location(0) position, @location(1) tex_coords (vertex.rs)
                vals = {by_loc[0]: W.Vec(F(x) for x in p), by_loc[1]: W.Vec(F(x) for x in uv)}
                outs.append(self.ns["fn_vs_main"](cls(*[vals[f] for f, _ in cls.FIELDS])))
        fpos, floc = self._io_fields(ret[0])
        tris = []
        for o in outs:
            p, uv = getattr(o, fpos), getattr(o, floc)
            assert len(p.c) == 4 and p.c[3] == F(1.0), "w = 1: no perspective division"
            assert uv.c[0] == (p.c[0] + F(1.0)) / F(2.0) and uv.c[1] == (F(1.0) - p.c[1]) / F(2.0), "uv is not the top-left-origin affine map of clip space"
            tris.append((float(p.c[0]), float(p.c[1])))
        assert len(tris) % 3 == 0
        tris = [tris[i:i + 3] for i in range(0, len(tris), 3)]

        def inside(t, q):
            s = []
            for i in range(3):
                (ax, ay), (bx, by) = t[i], t[(i + 1) % 3]
                s.append((bx - ax) * (q[1] - ay) - (by - ay) * (q[0] - ax))
            return all(v >= 0 for v in s) or all(v <= 0 for v in s)
        for q in [(-1, -1), (1, -1), (-1, 1), (1, 1), (0, 0), (-0.99, 0.99), (0.99, -0.99), (0.5, 0.25), (-0.25, -0.5)]:
            assert any(inside(t, q) for t in tris), "the drawn triangles do not cover the viewport"
        return len(outs)

    def fragment(self, x, y, tw, th):
        _, _, params, _, _ = self.fn["fs_main"]
        sname = params[0][1][0]
        cls = self.ns["S_" + sname]
        fpos, floc = self._io_fields(sname)
        px, py = F(x) + F(0.5), F(y) + F(0.5)
        vals = {fpos: W.Vec((px, py, F(0.0), F(1.0))), floc: W.Vec((px / F(tw), py / F(th)))}
        return self.ns["fn_fs_main"](cls(*[vals[f] for f, _ in cls.FIELDS]))

    def run(self, target, resources, src_size, rows=None, pixels=None):
        """fs_main over a (W', H') target (all of it, a band of rows, or the listed (x, y) pixels): float32 (H', W', 4) or (n, 4)."""
        tw, th = target
        self.bind(resources)
        self.sampler.scale = max(src_size[0] / tw, src_size[1] / th)
        with np.errstate(all="ignore"):
            if pixels is not None:
                out = np.empty((len(pixels), 4), np.float32)
                for i, (x, y) in enumerate(pixels):
                    out[i] = self.fragment(int(x), int(y), tw, th).c
                return out
            y0, y1 = rows if rows is not None else (0, th)
            out = np.empty((y1 - y0, tw, 4), np.float32)
            for y in range(y0, y1):
                for x in range(tw):
                    out[y - y0, x] = self.fragment(x, y, tw, th).c
        return out

    # -- coverage
    def counts(self):
        return self.ns["_HIT"], self.ns["_BR"], self.ns["_SEL"]

    def reset_counts(self):
        for c in self.counts():
            c.clear()

    def sites(self):
        """(statements, conditions, selects): token indices of every counted site of every function of the file"""
        st = sorted(i for v in self.ns["__sites__"]["stmt"].values() for i in v)
        br = sorted(i for v in self.ns["__sites__"]["cond"].values() for i in v)
        se = sorted(i for v in self.ns["__sites__"]["select"].values() for i in v)
        return st, br, se


# ------------------------------------------------------------------------------------------------------------------ the pipelines' data
def bloom_plan():
    """(pass count per direction, scale factor) from mod.rs, and the quad's (position, tex_coords) vertices from quad.rs - read as data"""
    mod = open(os.path.join(REF, "mod.rs")).read()
    count = int(re.search(r"let\s+bloom_pipeline_count\s*=\s*(\d+)\s*;", mod).group(1))
    mult = float(re.search(r"let\s+bloom_multiplier\s*=\s*([0-9.]+)\s*;", mod).group(1))
    pipe = open(os.path.join(REF, "pipelines", "bloom_pipline.rs")).read()
    args = [float(v) for v in re.search(r"Quad::new\(\s*([^)]*)\)", pipe).group(1).split(",")]
    quad = open(os.path.join(REF, "quad.rs")).read()
    env = dict(zip("xywh", (F(a) for a in args)))
    for name, e in re.findall(r"let\s+(\w+)\s*=\s*([^;]+);", quad):
        assert re.fullmatch(r"[\sxywh0-9.+\-*()]+", e) and "**" not in e, e     # + - * and parentheses only: the same in Rust and here
        env[name] = F(eval(e, {"__builtins__": {}}, dict(env)))                # f32 arithmetic, as the Rust lines are
    verts = []
    for p, t in re.findall(r"position:\s*\[([^\]]*)\]\s*,\s*tex_coords:\s*\[([^\]]*)\]", quad):
        num = lambda s: env[s.strip()] if s.strip() in env else F(float(s))   # noqa: E731
        verts.append(([num(s) for s in p.split(",")], [num(s) for s in t.split(",")]))
    assert len(verts) == 6
    if tuple(args) == (0.0, 0.0, 1.0, 1.0):                                       # the whole target: the four clip-space corners, uv 0 / 1
        assert {(float(p[0]), float(p[1]), float(p[2])) for p, _ in verts} == {(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (1.0, 1.0, 0.0), (-1.0, 1.0, 0.0)}
        assert all(float(v) in (0.0, 1.0) for _, t in verts for v in t)
    return count, mult, verts


def bloom_sizes(w, h, count=5, mult=2.0):
    """mod.rs:219-256: the f32 `current_res` divided `count` times, then multiplied `count` times; each target is `as u32` of the float"""
    cw, ch, out = F(w), F(h), []
    for i in range(2 * count):
        cw, ch = (cw / F(mult), ch / F(mult)) if i < count else (cw * F(mult), ch * F(mult))
        out.append((int(cw), int(ch)))
    return out


# ------------------------------------------------------------------------------------------------------------------ the 8-bit target
def srgb8(v):
    """Rgba8UnormSrgb store of linear values, from the definition in binary64 (R4)"""
    c = np.clip(np.asarray(v, dtype=np.float64), 0.0, 1.0)
    e = np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(c, 1.0 / 2.4) - 0.055)
    return np.floor(255.0 * e + 0.5).astype(np.uint8)


def unorm8(a):
    a = np.asarray(a, dtype=np.float32)
    return np.rint(np.where(a > F(0.0), np.where(a < F(1.0), a, F(1.0)), F(0.0)) * F(255.0)).astype(np.uint8)


def encode_rgba8(fxaa):
    out = np.empty(fxaa.shape, np.uint8)
    out[..., :3] = srgb8(fxaa[..., :3])
    out[..., 3] = unorm8(fxaa[..., 3])
    return out


def to16(img):
    with np.errstate(over="ignore"):
        return np.asarray(img, dtype=np.float32).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------ the pass runner
class Pipeline:
    """The five shaders compiled once, their vertex stages run and checked; sources = {stage: text} overrides a file (mutations)."""

    def __init__(self, sources=None):
        sources = sources or {}
        self.count, self.mult, self.quad = bloom_plan()
        self.sh = {s: Shader(s, sources.get(s)) for s in STAGES}
        for s in STAGES:
            self.sh[s].vertex_stage(self.quad if s in ("down", "up") else None)

    def stage_inputs(self, stage_index, sky16, levels, mix16, hdr16, fxaa_bytes, mix_bytes):
        """(stage, target size, resources, source size) of pass k: 0..2*count-1 the bloom passes, then mix, hdr, fxaa"""
        h, w = sky16.shape[:2]
        n = 2 * self.count
        sizes = bloom_sizes(w, h, self.count, self.mult)
        if stage_index < n:
            src = sky16 if stage_index == 0 else levels[stage_index - 1]
            return ("down" if stage_index < self.count else "up"), sizes[stage_index], {0: texture16(src)}, (src.shape[1], src.shape[0])
        if stage_index == n:
            assert sizes[-1] == (w, h)
            return "mix", (w, h), {1: texture16(sky16), 2: texture16(levels[-1]), 3: bytes(mix_bytes)}, (w, h)
        if stage_index == n + 1:
            return "hdr", (w, h), {0: texture16(mix16)}, (w, h)
        return "fxaa", (w, h), {0: texture16(hdr16), 2: bytes(fxaa_bytes)}, (w, h)

    def run_stage(self, stage_index, sky16, levels, mix16, hdr16, fxaa_bytes, mix_bytes, pixels=None, pool=None):
        stage, target, res, src_size = self.stage_inputs(stage_index, sky16, levels, mix16, hdr16, fxaa_bytes, mix_bytes)
        sh = self.sh[stage]
        if pool is None or pixels is not None or target[1] < 4:
            return sh.run(target, res, src_size, pixels=pixels)
        global _JOB
        _JOB = (sh, target, res, src_size)
        out = np.empty((target[1], target[0], 4), np.float32)
        step = max(1, -(-target[1] // (pool * 2)))
        import multiprocessing as mp
        with mp.get_context("fork").Pool(pool) as p:                        # forked here: the workers see _JOB
            for (y0, y1), part, cnt in p.imap_unordered(_band, [(y, min(target[1], y + step)) for y in range(0, target[1], step)]):
                out[y0:y1] = part
                for mine, theirs in zip(sh.counts(), cnt):
                    mine.update(theirs)
        return out

    def render_post(self, sky16, fxaa_bytes=FXAA_DEFAULT, mix_bytes=MIX_DEFAULT, processes=0):
        sky16 = np.asarray(sky16)
        sky16 = sky16.view(np.float16) if sky16.dtype == np.uint16 else sky16
        assert sky16.dtype == np.float16
        pool = processes if processes > 1 else None                          # rows of a pass spread over that many forked workers
        levels, mix16, hdr16 = [], None, None
        n = 2 * self.count
        for k in range(n):
            levels.append(to16(self.run_stage(k, sky16, levels, None, None, fxaa_bytes, mix_bytes, pool=pool)))
        mix16 = to16(self.run_stage(n, sky16, levels, None, None, fxaa_bytes, mix_bytes, pool=pool))
        hdr16 = to16(self.run_stage(n + 1, sky16, levels, mix16, None, fxaa_bytes, mix_bytes, pool=pool))
        fxaa = self.run_stage(n + 2, sky16, levels, mix16, hdr16, fxaa_bytes, mix_bytes, pool=pool)
        return dict(levels=levels, mix=mix16, hdr=hdr16, fxaa=fxaa, rgba8=encode_rgba8(fxaa))

    def coverage(self):
        """{stage: dict(stmt_tok, stmt_hits, cond_tok, cond_true, cond_false, sel_tok, sel_true, sel_false)} as int64 arrays"""
        out = {}
        for s in STAGES:
            sh = self.sh[s]
            hit, br, sel = sh.counts()
            st, cd, se = sh.sites()
            out[s] = dict(stmt_tok=np.array(st, np.int64), stmt_hits=np.array([hit[i] for i in st], np.int64),
                          cond_tok=np.array(cd, np.int64), cond_true=np.array([br[(i, True)] for i in cd], np.int64),
                          cond_false=np.array([br[(i, False)] for i in cd], np.int64),
                          sel_tok=np.array(se, np.int64), sel_true=np.array([sel[(i, True)] for i in se], np.int64),
                          sel_false=np.array([sel[(i, False)] for i in se], np.int64))
        return out

    def first_condition_false(self, stage="fxaa", fn="fs_main"):
        """how often the first `if` of a function was not taken: for fxaa.wgsl's fs_main, the fragments that pass the early exit"""
        idx = min(self.sh[stage].ns["__sites__"]["cond"][fn])
        return self.sh[stage].counts()[1][(idx, False)]


_JOB = None


def _band(rows):
    sh, target, res, src_size = _JOB
    sh.reset_counts()
    part = sh.run(target, res, src_size, rows=rows)
    return rows, part, tuple(collections.Counter(c) for c in sh.counts())


_PIPELINE = None


def render_post(sky16, fxaa_bytes=FXAA_DEFAULT, mix_bytes=MIX_DEFAULT, processes=0):
    """The display pass of one frame by the executed shader text: sky16 is the RGBA16F sky image (H x W x 4 float16 or its uint16 view),
    the uniforms their raw bytes (16 B FXAADetailsUniform, 4 B MixDetails).  Returns dict(levels = the 10 bloom targets, mix, hdr: float16
    (h, w, 4); fxaa: float32 (H, W, 4); rgba8: uint8 (H, W, 4)).  Hit counts accumulate in pipeline().coverage()."""
    return pipeline().render_post(sky16, fxaa_bytes, mix_bytes, processes)


def pipeline():
    global _PIPELINE
    if _PIPELINE is None:
        _PIPELINE = Pipeline()
    return _PIPELINE
