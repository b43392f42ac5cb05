"""-m gpu: bhray_timing under each shape of a batch's launch plan.

The plan (bhray_api.hip, BatchPlan) says which timing events stand around which launch, and bhray_get_timing decodes them; only the plain
ladder's counts are asserted elsewhere (test_gpu_parity.py).  Here: the plain ladder, the speculative levels' merged launch, the superset
launch, both, and the temporal mode - a four-level ladder, one frame per batch, one frame slot, three frames.  The expected counts were
recorded from this test run against a library built from the commit before the plan was restructured (profiles/r14_plan_timing_parent.txt;
it passes there unchanged); they are per batch x 3 batches:
classify 4 in every mode; trace launches timed as a level's own 4 / 3 / 3 / 2 / 4; predicted launches 0 / 0 / 0 / 0 / 1; execution spans
(every trace launch, the predicted one included) 4 / 3 / 3 / 2 / 5."""
import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T

pytestmark = pytest.mark.gpu

FRAMES, LEVELS = 3, 4
# mode -> (RayPass keywords, levels with a trace launch of their own, (classify, trace, predicted, execution spans) of the three batches)
MODES = {
    "plain": ({}, (0, 1, 2, 3), (12, 12, 0, 12)),
    "speculative": ({"speculative_levels": 2}, (0, 2, 3), (12, 9, 0, 9)),        # level 1 is classified against the merged launch's image
    "superset": ({"superset_levels": 2}, (0, 1, 2), (12, 9, 0, 9)),              # levels 2 and 3 in one launch, timed as level 2's
    "speculative+superset": ({"speculative_levels": 2, "superset_levels": 2}, (0, 2), (12, 6, 0, 6)),
    "temporal": ({"temporal": True}, (0, 1, 2, 3), (12, 12, 3, 15)),             # the predicted launch, then a fix-up pair per level
}


def _run(kw):
    rp = B.RayPass(B.ladder_from_base((24, 14), 3, LEVELS), device=0, timing=True, frames_per_batch=1, frames_in_flight=1, **kw)
    rp.set_textures(*T.textures())
    rp.set_uniforms(*T.uniforms(integration_method=1))
    for _ in range(FRAMES):
        rp.render()
    t = rp.timing()
    return t, rp.read_hdr()


@pytest.fixture(scope="module")
def plain_frame():
    frame = _run({})[1]
    frame.setflags(write=False)
    return frame


@pytest.mark.parametrize("mode", list(MODES))
def test_timing_counts_and_level_intervals(mode, plain_frame):
    kw, own_trace, counts = MODES[mode]
    t, frame = _run(kw)
    print(mode, "frames", t.frames, "batches", t.batches, "classify", t.classify_launches, "trace", t.trace_launches, "predicted", t.predicted_launches,
          "exec", t.trace_exec_launches, "level_trace_ms", list(t.level_trace_ms)[:LEVELS], "total_ms", t.total_ms, "trace_ms", t.trace_ms)
    assert (t.frames, t.batches) == (FRAMES, FRAMES)
    assert (t.classify_launches, t.trace_launches, t.predicted_launches, t.trace_exec_launches) == counts
    for l in range(LEVELS):
        if l in own_trace:
            assert t.level_trace_ms[l] > 0, f"level {l}"
        else:
            assert t.level_trace_ms[l] == 0, f"level {l} has no trace launch of its own"
    assert t.total_ms >= t.trace_ms
    assert np.array_equal(frame.view(np.uint32), plain_frame.view(np.uint32)), "the final frame differs from the plain ladder's"
