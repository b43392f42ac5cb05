"""Cost of the point-star pass against the starless sky pass of the same run.

`python profiles/stars_cost.py` renders 1920x1080 frames of the default scene (RK, the large textures: a 4096x2048 sky) on one ctx with BHRAY_F_TIMING and
sets and removes a catalogue of 120 000 seeded stars (G = 128) in alternating blocks of 20 frames; each frame is rendered, resolved and synchronised on its own, and
its sky pass's time is the span between the two events the library records around the pass (bhray_timing.sky_ms) - the sky kernel and, with a catalogue, the star
kernel behind it.  Prints one JSON object: the median per mode over all blocks (the first two frames of a block are dropped), their ratio, and - from the host form
of the rule over one frame of the device (bhray_diag_stars_pixel_info_host) - the pixels with a footprint, those skipped by size and by cells, the pixels that
received a star and the mean number of stars the inside test ran on per pixel with a footprint."""
import json
import os
import statistics
import sys

BLOCKS, FRAMES, DROP = 6, 20, 2
STARS, SEED = 120000, 1


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bhusie_amd as B
    from bhusie_amd import assets
    from tests import common as T
    tex = T.textures(small=False)
    cat = assets.star_catalogue(STARS, SEED)
    rp = B.RayPass(B.ladder_for_frame((1920, 1080), 3, 4), device=0, timing=True)
    rp.set_textures(*tex)
    rp.set_uniforms(*T.uniforms(integration_method=1))
    us = {0: [], 1: []}
    blocks = []
    for b in range(BLOCKS):
        mode = b % 2
        rp.set_stars(cat if mode else None)
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
    info = B.stars_pixel_info_host(frame, cat)
    fp = info["state"] != 3
    off, on = statistics.median(us[0]), statistics.median(us[1])
    print(json.dumps({
        "source": "BHRAY_F_TIMING sky span, 1920x1080, default scene, RK, 4096x2048 sky, 120000 seeded stars (G = 128); alternating blocks of 20 frames on one ctx, first 2 of a block dropped",
        "sky_pass_without_stars_us": round(off, 2), "sky_pass_with_stars_us": round(on, 2), "ratio_with_over_without": round(on / off, 3), "blocks": blocks,
        "pixels": int(fp.size), "with_footprint": int(fp.sum()), "skipped_by_size": int((info["state"] == 1).sum()), "skipped_by_cells": int((info["state"] == 2).sum()),
        "received_a_star": int((info["accepted"] > 0).sum()), "through_the_reversed_form": int((info["reversed"] > 0).sum()),
        "mean_stars_tested_per_footprint_pixel": round(float(info["tested"].sum()) / max(int(fp.sum()), 1), 3), "max_stars_tested": int(info["tested"].max()),
        "mean_cells_per_footprint_pixel": round(float(info["cells"].sum()) / max(int(fp.sum()), 1), 3)}))


if __name__ == "__main__":
    main()
