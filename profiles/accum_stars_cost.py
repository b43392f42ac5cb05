"""Cost of point stars in stills against the starless still of the same run.

`python profiles/accum_stars_cost.py` accumulates 1920x1080 stills of 16 samples of the default scene (RK, the large textures: a 4096x2048 sky) on one ctx that holds
a catalogue of 120 000 seeded stars (G = 128, §23's), with bhray_accum_set_stars off and on in alternating blocks of 6 stills.  A still is timed on the host from
accum_begin to the return of accum_read and divided by its 16 samples; the first still of a block is dropped.  Prints one JSON object: the median ms per sample per
mode over all blocks, their difference in microseconds, and the blocks' own medians."""
import json
import os
import statistics
import sys
import time

BLOCKS, STILLS, DROP, SAMPLES = 6, 6, 1, 16
STARS, SEED = 120000, 1


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bhusie_amd as B
    from bhusie_amd import assets
    from tests import common as T
    rp = B.RayPass(B.ladder_for_frame((1920, 1080), 3, 4), device=0)
    rp.set_textures(*T.textures(small=False))
    rp.set_uniforms(*T.uniforms(integration_method=1))
    rp.set_stars(assets.star_catalogue(STARS, SEED))
    ms = {0: [], 1: []}
    blocks = []
    images = {}
    for b in range(BLOCKS):
        mode = b % 2
        rp.accum_set_stars(bool(mode))
        mine = []
        for _ in range(STILLS):
            t0 = time.perf_counter()
            rp.accum_begin()
            rp.accum_add(SAMPLES)
            images[mode] = rp.accum_read()
            mine.append(1e3 * (time.perf_counter() - t0) / SAMPLES)
        ms[mode] += mine[DROP:]
        blocks.append({"mode": mode, "median_ms_per_sample": round(statistics.median(mine[DROP:]), 4), "min": round(min(mine), 4), "max": round(max(mine), 4)})
    rp.close()
    changed = int((images[0].view("uint32") != images[1].view("uint32")).any(axis=-1).sum())
    off, on = statistics.median(ms[0]), statistics.median(ms[1])
    print(json.dumps({
        "source": "host clock from accum_begin to the return of accum_read over 16, 1920x1080, default scene, RK, 4096x2048 sky, 120000 seeded stars (G = 128); "
                  "bhray_accum_set_stars off and on in alternating blocks of 6 stills on one ctx, the first of a block dropped",
        "ms_per_sample_without_stars": round(off, 4), "ms_per_sample_with_stars": round(on, 4), "difference_us_per_sample": round(1e3 * (on - off), 1),
        "ratio_with_over_without": round(on / off, 4), "blocks": blocks, "pixels_of_the_mean_changed": changed}))


if __name__ == "__main__":
    main()
