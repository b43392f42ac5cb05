"""Blocks the ladder's trace launches get per frame of the flagship workload (1920x1080, adaptive RK, 22 frame slots, two speculative levels), with the trace grids sized by
queue length and with BHRAY_LEVEL_GRID=0: bhray_get_level_grids after 10 rounds of the slots (EXPERIMENTS R13.1).  usage: python profiles/jobs/level_grid_blocks.py"""
import os
import sys

os.environ["GPU_MAX_HW_QUEUES"] = "32"            # as bench.py: one stream per frame slot
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bhusie_amd as B                            # noqa: E402
from bhusie_amd import assets                     # noqa: E402

tex = assets.temp_lut(256), assets.disk_texture(1000, seed=1), assets.sky_texture(4096, 2048, seed=2)
cfg = B.ladder_for_frame((1920, 1080), 3, 4)
for rule in ("1", "0"):
    os.environ["BHRAY_LEVEL_GRID"] = rule
    rp = B.RayPass(cfg, device=0, frames_in_flight=22, speculative_levels=2)
    rp.set_textures(*tex)
    frames = 220
    for k in range(frames):
        rp.set_uniforms(B.Camera().uniform(), B.BlackHole().uniform(), B.RayDetails(integration_method=1, time=k / 60.0).uniform())
        rp.render()
    rp.sync()
    g = rp.level_grids((frames - 1) % 22)
    print(f"BHRAY_LEVEL_GRID={rule}: ctx grid {g['ctx_grid']}, dense {g['dense']}, last batch (blocks, expected rays) {g['launches']}; {g['total_launches']} trace launches, "
          f"{g['total_blocks']} blocks = {g['total_blocks'] / frames:.0f} per frame, {g['total_ceiling_launches']} launches at the ceiling")
    rp.close()
