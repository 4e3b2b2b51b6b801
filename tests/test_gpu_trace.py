"""The determinism trace of match() (option "trace", roma_debug_trace) is an interface of tools/stress_streams.py,
tools/repro_mixed.py and tools/schedule_dump.py: the ordered stage names of a call are pinned to
tests/golden/trace_stage_names.json (written by `tools/schedule_dump.py --golden`), and two identical calls must give
identical checksums."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_trace_stage_names_and_repeatability(built_lib, weights0, mode):
    from roma_amd import roma_model, synthetic
    sd, dsd = weights0
    golden = json.load(open(os.path.join(GOLDEN, "trace_stage_names.json")))[mode]
    inp = {k: v.cuda() for k, v in synthetic.make_inputs(2, 112, 168, seed=7).items()}
    m = roma_model((112, 112), True, device="cuda:0", weights=sd, dinov2_weights=dsd, symmetric=True, upsample_res=(168, 168),
                   amp_dtype=torch.float32 if mode == "f32" else torch.bfloat16, max_batch=2)  # fused refiner blocks: the default
    m.trace = True
    runs = []
    for _ in range(3):
        m.match(inp["im_A"], inp["im_B"], im_A_high_res=inp["im_A_high_res"], im_B_high_res=inp["im_B_high_res"])
        torch.cuda.synchronize()
        runs.append([m.debug_trace(slot) for slot in (0, 1)])  # two pairs: one per sub-batch stream
    names0, sums0 = runs[0][0]
    assert list(names0) == golden, [(i, a, b) for i, (a, b) in enumerate(zip(names0, golden)) if a != b][:5]
    assert len(sums0) == len(golden) and np.count_nonzero(sums0) > len(golden) // 2

    def differing(a, b):
        assert list(a[0]) == list(b[0])
        return {n for n, x, y in zip(a[0], a[1], b[1]) if x != y}

    for slot in (0, 1):
        # The logits rows are 4104 floats wide and to_out writes 4100 of them; the checksum covers the row, so its four pad
        # columns show what the arena held before: zeros in the first call of a handle, the previous call's scratch afterwards.
        # cls_to_flow reads 4097 columns.  Every other stage is equal from the first call on.
        assert differing(runs[0][slot], runs[1][slot]) <= {"p1_s16_logits"}
        assert differing(runs[1][slot], runs[2][slot]) == set()
