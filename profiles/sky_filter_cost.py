"""Cost of the footprint-filtered sky pass against the unfiltered pass of the same run.

`python profiles/sky_filter_cost.py` renders 1920x1080 frames of the default scene (RK, the large textures: a 4096x2048 sky) on one ctx with BHRAY_F_TIMING and
switches the filter off and on in alternating blocks of 20 frames; each frame is rendered, resolved and synchronised on its own, and its sky pass's time is the
span between the two events the library records around the pass (bhray_timing.sky_ms).  Prints one JSON object: the median per mode over all blocks (the first two
frames of a block are dropped: the first pass after a switch meets a cold pyramid), their ratio, and - from the NumPy restatement over one frame of the device -
the share of direction pixels that are filtered, the tap histogram and the level histogram."""
import json
import os
import statistics
import sys

BLOCKS, FRAMES, DROP = 6, 20, 2


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bhusie_amd as B
    from tests import common as T
    from tests import sky_filter_ref as S
    tex = T.textures(small=False)
    rp = B.RayPass(B.ladder_for_frame((1920, 1080), 3, 4), device=0, timing=True)
    rp.set_textures(*tex)
    rp.set_uniforms(*T.uniforms(integration_method=1))
    us = {0: [], 1: []}
    blocks = []
    for b in range(BLOCKS):
        mode = b % 2
        rp.set_sky_filter(mode)
        mine = []
        for f in range(FRAMES):
            rp.render(); rp.sync()                               # the frame is done: the sky pass runs alone
            rp.resolve_sky(); rp.sync()
            t = rp.timing()                                      # the batches since the last call: this frame's
            assert t.sky_launches == 1, t.sky_launches
            mine.append(1e3 * float(t.sky_ms))
        us[mode] += mine[DROP:]
        blocks.append({"mode": mode, "median_us": round(statistics.median(mine[DROP:]), 2), "min_us": round(min(mine), 2), "max_us": round(max(mine), 2)})
    frame = rp.read_hdr()
    rp.close()
    _, st = S.resolve(frame, tex[2])
    off, on = statistics.median(us[0]), statistics.median(us[1])
    print(json.dumps({
        "source": "BHRAY_F_TIMING sky span, 1920x1080, default scene, RK, 4096x2048 sky; alternating blocks of 20 frames on one ctx, first 2 of a block dropped",
        "sky_pass_off_us": round(off, 2), "sky_pass_on_us": round(on, 2), "ratio_on_over_off": round(on / off, 3), "blocks": blocks,
        "direction_pixels": st["direction"], "filtered": st["filtered"], "filtered_share": round(st["filtered"] / max(st["direction"], 1), 4),
        "taps": st["taps"], "levels": st["levels"], "frac_nonzero": st["frac_nonzero"]}))


if __name__ == "__main__":
    main()
