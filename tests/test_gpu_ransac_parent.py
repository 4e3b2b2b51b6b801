"""Every instantiation of the shared RANSAC pipeline (csrc/ransac.h: H, F and E under count and MAGSAC++ scoring, absolute pose)
against the bits it produced before absolute pose became one of its model policies: tests/golden/ransac_parent.npz, written by
tools/record_ransac_parent.py at that commit.  The pipeline is deterministic, compiled with fp contract(off) and scores with
explicit fmaf, so the criterion is equality."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from ransac_parent_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(GOLDEN, "ransac_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(parent):
    assert {k.split("/")[0] for k in parent} == set(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bits_of_the_parent(built_lib, parent, case):
    out = CASES[case]()
    assert len(out) == sum(k.startswith(case + "/") for k in parent)
    for i, x in enumerate(out):
        want = torch.as_tensor(parent[f"{case}/{i}"])
        assert x.dtype == want.dtype and torch.equal(x.cpu(), want), (case, i)
