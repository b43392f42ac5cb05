"""Point stars in stills (bhray_accum_set_stars) restated in NumPy from include/bhray.h's contract: a sample's starred image T_s - §23's rules 1 - 6
(tests/stars_ref.resolve, unchanged) over the sample's trace results, the wrap of a whole equirect still by padding one column each side, and step 3 with
tests/accum_ref.resolve - and the mean of the starred images through tests/accum_ref.accumulate (the box) or tests/accum_filter_ref.accumulate (tent, cubic).  What
tests/test_accum_stars_cpu.py and tests/test_gpu_accum_stars.py compare with."""
from __future__ import annotations

import numpy as np

from tests import accum_filter_ref as FR
from tests import accum_ref as A
from tests import stars_ref as S

F = np.float32
CAP = F(65504.0)


def star_sum(results_hw4, stars, params=None, wrap_x=False):
    """steps 1 and 2: (add, st) of stars_ref.resolve over the (h, w, 4) sample image; wrap_x: column -1 is column w - 1 and column w is column 0 (the per-pixel arrays
    of st are cropped to the frame; st["hits"] is given in frame coordinates)"""
    r = np.asarray(results_hw4, F)
    kw = dict(params or {})
    if not wrap_x:
        return S.resolve(r, stars, **kw)
    padded = np.concatenate([r[:, -1:], r, r[:, :1]], axis=1)
    add, st = S.resolve(padded, stars, **kw)
    out = {k: (v[:, 1:-1] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    out["hits"] = [(y, x - 1, k, rev) for y, x, k, rev in st["hits"] if 1 <= x <= r.shape[1]]
    return np.ascontiguousarray(add[:, 1:-1]), out


def starred(results_hw4, stars, params, t_sky, wrap_x=False):
    """(T, add, st): step 3 - a pixel that accepted a star becomes (min(b + acc * gain, 65504), 1), b the accumulation's resolve of the pixel; every other pixel keeps
    its bits.  params: None or a dict of gain, min_area, max_footprint"""
    r = np.asarray(results_hw4, F)
    add, st = star_sum(r, stars, params, wrap_x)
    T = r.copy()
    lit = add[..., 3] > 0
    if lit.any():
        b = A.resolve(r[lit], t_sky)
        assert (b[:, 3] == 1).all()
        with np.errstate(over="ignore", invalid="ignore"):
            v = (b[:, 0:3] + add[lit][:, 0:3]).astype(F)
            v = np.where(CAP < v, CAP, v).astype(F)                  # min_(a, b) = b < a ? b : a
        T[lit] = np.concatenate([v, np.ones((v.shape[0], 1), F)], axis=1)
    return T, add, st


def mean(starred_images, t_sky, filt: FR.Filter | None = None, s0: int = 0):
    """(mean, total): step 4 - the starred images of samples s0, s0 + 1, ... where the trace results were: accum_ref.accumulate under the box, accum_filter_ref.accumulate
    under a tent or a cubic; (h * w, 4) each"""
    imgs = [np.asarray(t, F) for t in starred_images]
    h, w = imgs[0].shape[0:2]
    flat = [t.reshape(-1, 4) for t in imgs]
    if filt is None or filt.kind == FR.BOX:
        total = A.accumulate(flat, t_sky)
    else:
        total = FR.accumulate(flat, t_sky, filt, w, h, s0)
    return A.mean(total), total
