"""NumPy restatement of the reference's display pass: bloom_down.wgsl, bloom_up.wgsl, mix.wgsl, hdr.wgsl and fxaa.wgsl (all under
/src/renderer/shaders of the reference), wired as src/renderer/mod.rs:209-324 wires them, under the rules of DESIGN.md §10.

Written from the WGSL text, not from the kernels.  float32 throughout (every constant is an np.float32, every operation in the shader's
order), np.float16 for the Rgba16Float targets, and the exact sRGB encoding of the Rgba8UnormSrgb target.  post_ref(sky) takes the
RGBA16F sky image (H x W x 4 float16) and returns the RGBA8 image (H x W x 4 uint8) that bhray_read_display delivers.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
F = lambda v: np.float32(v)     # noqa: E731  (a WGSL literal converted to f32)

FXAA_DEFAULT = (F(0.0156), F(0.063), 12, F(0.75))          # Renderer::render: EdgeThresholdMin/Max::Ultra, 12, 0.75
MIX_DEFAULT = F(0.7)                                        # mod.rs:258-260


def bloom_sizes(W: int, H: int):
    """mod.rs:219-256: the f32 `current_res` halved five times, then doubled five times; each target is (u32) of the float."""
    cw, ch = F(W), F(H)
    out = []
    for i in range(10):
        if i < 5:
            cw, ch = f32(cw / F(2.0)), f32(ch / F(2.0))
        else:
            cw, ch = f32(cw * F(2.0)), f32(ch * F(2.0))
        out.append((int(cw), int(ch)))
    if any(w == 0 or h == 0 for w, h in out):
        raise ValueError("a bloom level would be empty (W or H < 32)")
    return out


def frag_uv(w: int, h: int):
    """The fragment's texture coordinate at pixel (x, y) of a w x h target: ((x + 0.5) / w, (y + 0.5) / h), v = 0 on the top row."""
    u = (np.arange(w, dtype=f32) + F(0.5)) / F(w)
    v = (np.arange(h, dtype=f32) + F(0.5)) / F(h)
    return np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))


def nearest(img, u, v):
    """min filter Nearest, ClampToEdge: texel floor(u * n)"""
    h, w = img.shape[:2]
    xi = np.clip(np.floor(u * F(w)), 0, w - 1).astype(np.int64)
    yi = np.clip(np.floor(v * F(h)), 0, h - 1).astype(np.int64)
    return img[yi, xi]


def _coord(u, n, off):
    x = u * F(n) - F(0.5)
    x = x + F(off)
    x = np.where(~(x >= F(-1.0)), F(-1.0), x)
    x = np.where(x > F(n), F(n), x).astype(f32)
    fl = np.floor(x)
    a = np.clip(fl, 0, n - 1).astype(np.int64)
    b = np.clip(fl + F(1.0), 0, n - 1).astype(np.int64)
    return a, b, (x - fl)


def _mix(a, b, t):
    """WGSL mix(a, b, t) = a * (1 - t) + b * t"""
    return a * (F(1.0) - t) + b * t


def bilinear(img, u, v, ox=0, oy=0):
    """mag filter Linear, ClampToEdge; texel centres at +0.5; an integer offset is added to the texel coordinate after the -0.5."""
    h, w = img.shape[:2]
    x0, x1, fx = _coord(u, w, ox)
    y0, y1, fy = _coord(v, h, oy)
    fx, fy = fx[..., None], fy[..., None]
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    return _mix(_mix(a, b, fx), _mix(c, d, fx), fy)


def to16(x):
    """an Rgba16Float target: round to nearest even"""
    return np.asarray(x, dtype=f32).astype(np.float16).astype(f32)


def bloom_down(src, tw, th):
    """bloom_down.wgsl:fs_main; src is the previous level (rgb), the result is rounded to binary16"""
    u, v = frag_uv(tw, th)
    sh, sw = src.shape[:2]
    x = F(1.0) / F(sw)
    y = F(1.0) / F(sh)
    x2, y2 = F(2.0) * x, F(2.0) * y
    a = nearest(src, u - x2, v + y2); b = nearest(src, u, v + y2); c = nearest(src, u + x2, v + y2)
    d = nearest(src, u - x2, v);      e = nearest(src, u, v);      f = nearest(src, u + x2, v)
    g = nearest(src, u - x2, v - y2); h = nearest(src, u, v - y2); i = nearest(src, u + x2, v - y2)
    j = nearest(src, u - x, v + y);   k = nearest(src, u + x, v + y)
    l = nearest(src, u - x, v - y);   m = nearest(src, u + x, v - y)
    ds = e * F(0.125)
    ds = ds + (((a + c) + g) + i) * F(0.03125)
    ds = ds + (((b + d) + f) + h) * F(0.0625)
    ds = ds + (((j + k) + l) + m) * F(0.125)
    return to16(ds)


def bloom_up(src, tw, th):
    """bloom_up.wgsl:fs_main (offsets of 0.005 in uv); the result is rounded to binary16"""
    u, v = frag_uv(tw, th)
    o = F(0.005)
    um, up, vp, vm = u - o, u + o, v + o, v - o
    a = bilinear(src, um, vp); b = bilinear(src, u, vp); c = bilinear(src, up, vp)
    d = bilinear(src, um, v);  e = bilinear(src, u, v);  f = bilinear(src, up, v)
    g = bilinear(src, um, vm); h = bilinear(src, u, vm); i = bilinear(src, up, vm)
    us = e * F(4.0)
    us = us + (((b + d) + f) + h) * F(2.0)
    us = us + (((a + c) + g) + i)
    us = us * (F(1.0) / F(16.0))
    return to16(us)


def bloom(sky_rgb):
    """the 10 bloom passes over the sky image's rgb (alpha is 1.0 in every bloom target)"""
    H, W = sky_rgb.shape[:2]
    img = sky_rgb
    for i, (w, h) in enumerate(bloom_sizes(W, H)):
        img = bloom_down(img, w, h) if i < 5 else bloom_up(img, w, h)
    return img


M1 = np.array([[0.59719, 0.07600, 0.02840], [0.35458, 0.90834, 0.13383], [0.04823, 0.01566, 0.83777]], dtype=f32)   # columns
M2 = np.array([[1.60475, -0.10208, -0.00327], [-0.53108, 1.10813, -0.07276], [-0.07367, -0.00605, 1.07602]], dtype=f32)


def matvec(m, x):
    """WGSL mat3x3 * vec3, column-major: (c0 * x + c1 * y) + c2 * z"""
    return (m[0] * x[..., 0:1] + m[1] * x[..., 1:2]) + m[2] * x[..., 2:3]


def aces(hdr):
    """hdr.wgsl:aces_tone_map; clamp with maxNum / minNum semantics (NaN -> 0)"""
    hdr = np.asarray(hdr, dtype=f32)
    v = matvec(M1, hdr)
    a = v * (v + F(0.0245786)) - F(0.000090537)
    b = v * (F(0.983729) * v + F(0.4329510)) + F(0.238081)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = a / b
    return np.fmin(np.fmax(matvec(M2, q), F(0.0)), F(1.0))


def mix(sky, bloom_rgb, ratio):
    """mix.wgsl (r * sky + (1 - r) * bloom, alpha included: bloom alpha is 1.0) -> fp16"""
    r = F(ratio)
    r1 = F(1.0) - r
    bl = np.concatenate([bloom_rgb, np.ones(bloom_rgb.shape[:2] + (1,), dtype=f32)], axis=-1)
    return to16(r * sky + r1 * bl)


def hdr(mx):
    """hdr.wgsl over the mixed image -> fp16 (alpha kept)"""
    return to16(np.concatenate([aces(mx[..., :3]), mx[..., 3:4]], axis=-1))


def mix_hdr(sky, bloom_rgb, ratio):
    """mix.wgsl -> fp16, then hdr.wgsl -> fp16"""
    return hdr(mix(sky, bloom_rgb, ratio))


def luma(c):
    """fxaa.wgsl:rgb2luma = sqrt(dot(rgb, (0.299, 0.587, 0.114)))"""
    return np.sqrt((c[..., 0] * F(0.299) + c[..., 1] * F(0.587)) + c[..., 2] * F(0.114))


def quality(i: int):
    return F({5: 1.5, 6: 2.0, 7: 2.0, 8: 2.0, 9: 2.0, 10: 4.0, 11: 8.0}.get(i, 1.0))


def fxaa(tone, details=FXAA_DEFAULT):
    """fxaa.wgsl:fs_main over the tone-mapped image (H x W x 4 f32 holding binary16 values); returns linear RGBA (f32)."""
    emin, emax, iterations, subq = F(details[0]), F(details[1]), int(details[2]), F(details[3])
    H, W = tone.shape[:2]
    isx, isy = F(1.0) / F(W), F(1.0) / F(H)
    tcx = np.broadcast_to(((np.arange(W, dtype=f32) + F(0.5)) * isx)[None, :], (H, W)).reshape(-1)
    tcy = np.broadcast_to(((np.arange(H, dtype=f32) + F(0.5)) * isy)[:, None], (H, W)).reshape(-1)
    S = lambda u, v, ox=0, oy=0: bilinear(tone, u, v, ox, oy)   # noqa: E731
    center = S(tcx, tcy)
    out = center.copy()
    lC = luma(center)
    lD, lU, lL, lR = luma(S(tcx, tcy, 0, -1)), luma(S(tcx, tcy, 0, 1)), luma(S(tcx, tcy, -1, 0)), luma(S(tcx, tcy, 1, 0))
    lMin = np.minimum(lC, np.minimum(np.minimum(lD, lU), np.minimum(lL, lR)))
    lMax = np.maximum(lC, np.maximum(np.maximum(lD, lU), np.maximum(lL, lR)))
    lRange = lMax - lMin
    go = ~(lRange < np.maximum(emin, lMax * emax))              # pixels past the early exit
    idx = np.nonzero(go)[0]
    if idx.size:
        tx, ty = tcx[idx], tcy[idx]
        lC, lD, lU, lL, lR, lRange = lC[idx], lD[idx], lU[idx], lL[idx], lR[idx], lRange[idx]
        lDL, lUR = luma(S(tx, ty, -1, -1)), luma(S(tx, ty, 1, 1))
        lUL, lDR = luma(S(tx, ty, -1, 1)), luma(S(tx, ty, 1, -1))
        lDU, lLR = lD + lU, lL + lR
        lLC, lDC, lRC, lUC = lDL + lUL, lDL + lDR, lDR + lUR, lUR + lUL
        eH = (np.abs(F(-2.0) * lL + lLC) + np.abs(F(-2.0) * lC + lDU) * F(2.0)) + np.abs(F(-2.0) * lR + lRC)
        eV = (np.abs(F(-2.0) * lU + lUC) + np.abs(F(-2.0) * lC + lLR) * F(2.0)) + np.abs(F(-2.0) * lD + lDC)
        isH = eH >= eV
        step = np.where(isH, isy, isx).astype(f32)
        l1 = np.where(isH, lD, lL)
        l2 = np.where(isH, lU, lR)
        g1, g2 = l1 - lC, l2 - lC
        steep1 = np.abs(g1) >= np.abs(g2)
        gScaled = F(0.25) * np.maximum(np.abs(g1), np.abs(g2))
        step = np.where(steep1, -step, step)
        lAvg = np.where(steep1, F(0.5) * (l1 + lC), F(0.5) * (l2 + lC))
        cux = np.where(isH, tx, tx + step * F(0.5))
        cuy = np.where(isH, ty + step * F(0.5), ty)
        ofx = np.where(isH, isx, F(0.0)).astype(f32)
        ofy = np.where(isH, F(0.0), isy).astype(f32)
        u1x, u1y, u2x, u2y = cux - ofx, cuy - ofy, cux + ofx, cuy + ofy
        e1 = luma(S(u1x, u1y)) - lAvg
        e2 = luma(S(u2x, u2y)) - lAvg
        r1, r2 = np.abs(e1) >= gScaled, np.abs(e2) >= gScaled
        both = r1 & r2
        u1x, u1y = np.where(r1, u1x, u1x - ofx), np.where(r1, u1y, u1y - ofy)
        u2x, u2y = np.where(r2, u2x, u2x - ofx), np.where(r2, u2y, u2y - ofy)   # fxaa.wgsl:132: `uv2 - offset`, as the text has it
        run = ~both                                              # pixels inside the search loop
        for i in range(2, iterations):
            if not run.any():
                break
            m1 = run & ~r1
            if m1.any():
                e1[m1] = luma(S(u1x[m1], u1y[m1])) - lAvg[m1]
            m2 = run & ~r2
            if m2.any():
                e2[m2] = luma(S(u2x[m2], u2y[m2])) - lAvg[m2]
            r1 = np.where(run, np.abs(e1) >= gScaled, r1)
            r2 = np.where(run, np.abs(e2) >= gScaled, r2)
            both = r1 & r2
            q = quality(i)
            m1, m2 = run & ~r1, run & ~r2
            u1x = np.where(m1, u1x - ofx * q, u1x); u1y = np.where(m1, u1y - ofy * q, u1y)
            u2x = np.where(m2, u2x + ofx * q, u2x); u2y = np.where(m2, u2y + ofy * q, u2y)
            run = run & ~both
        d1 = np.where(isH, tx - u1x, ty - u1y)
        d2 = np.where(isH, u2x - tx, u2y - ty)
        dir1 = d1 < d2
        dFinal = np.minimum(d1, d2)
        thick = d1 + d2
        cSmaller = lC < lAvg
        cv1 = (e1 < F(0.0)) != cSmaller
        cv2 = (e2 < F(0.0)) != cSmaller
        cv = np.where(dir1, cv1, cv2)
        with np.errstate(invalid="ignore", divide="ignore"):
            pixOff = (-dFinal) / thick + F(0.5)
            fin = np.where(cv, pixOff, F(0.0)).astype(f32)
            lAverage = F(1.0 / 12.0) * (((F(2.0) * (lDU + lLR)) + lLC) + lRC)
            s1 = np.fmin(np.fmax(np.abs(lAverage - lC) / lRange, F(0.0)), F(1.0))
        s2 = ((F(-2.0) * s1 + F(3.0)) * s1) * s1
        sFinal = (s2 * s2) * subq
        fin = np.maximum(fin, sFinal)
        fux = np.where(isH, tx, tx + fin * step)
        fuy = np.where(isH, ty + fin * step, ty)
        fc = S(fux, fuy)
        out[idx, :3] = fc[:, :3]
    return out.reshape(H, W, 4)


def srgb_thresholds():
    """t_k = srgb_decode((k - 0.5) / 255), k = 1..255, in double, rounded UP to f32 (the smallest f32 >= the threshold, so that for every
    f32 value: value >= t_k <=> value >= the double threshold): byte >= k <=> value >= t_k"""
    c = (np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    t = lin.astype(f32)
    return np.where(t.astype(np.float64) < lin, np.nextafter(t, f32(np.inf)), t).astype(f32)


_THR = srgb_thresholds()


def srgb_encode(v):
    """Rgba8UnormSrgb store of linear values: the number of thresholds <= v (NaN -> 0)"""
    v = np.asarray(v, dtype=f32)
    b = np.searchsorted(_THR, np.nan_to_num(v, nan=-1.0), side="right")
    return b.astype(np.uint8)


def unorm8(a):
    a = np.asarray(a, dtype=f32)
    b = np.rint(np.clip(np.nan_to_num(a, nan=0.0), F(0.0), F(1.0)) * F(255.0))
    return b.astype(np.uint8)


def tone_map(sky, mix_ratio=MIX_DEFAULT):
    """bloom, mix, hdr: the tone-mapped Rgba16Float image (f32 holding binary16 values)"""
    s = np.asarray(sky, dtype=np.float16).astype(f32)
    return mix_hdr(s, bloom(s[..., :3]), mix_ratio)


def post_ref(sky, fxaa_details=FXAA_DEFAULT, mix_ratio=MIX_DEFAULT):
    """RGBA16F sky image (H x W x 4) -> the RGBA8 image of the FXAA target"""
    c = fxaa(tone_map(sky, mix_ratio), fxaa_details)
    out = np.empty(c.shape, dtype=np.uint8)
    out[..., :3] = srgb_encode(c[..., :3])
    out[..., 3] = unorm8(c[..., 3])
    return out
