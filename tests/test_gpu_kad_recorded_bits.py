"""The Kernel Audio Distance family computes the bits recorded in tests/golden/kad_bits.npz: the outputs of the order
statistic, the whole-set sums (one and several scales), the two-sided row sums and the per-group sums, f32 and f64, from an
earlier library on the MI355X (tests/golden/make_goldens_kad.py lists the calls and says why each shape is there).  No
tolerance: float64 results are compared as int64, so a NaN compares too and one differing bit fails."""
import os

import numpy as np
import pytest
import torch

import make_goldens_kad as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with np.load(rec.BITS_NPZ, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_every_recorded_array_belongs_to_a_case(recorded):
    names = [c[0] for c in rec.SHAPES]
    assert recorded and all(k.split("__")[0] in names for k in recorded), sorted(recorded)


@pytest.mark.parametrize("case", rec.SHAPES, ids=[c[0] for c in rec.SHAPES])
def test_outputs_are_the_recorded_bits(case, recorded):
    import audio_metrics_amd as am
    got = rec.bits_of(case, am.hip_ops, torch)
    want = {k: v for k, v in recorded.items() if k.split("__")[0] == case[0]}
    assert sorted(got) == sorted(want) and len(got) >= 10
    wrong = []
    for k in sorted(got):
        w = torch.from_numpy(want[k])
        assert got[k].dtype == w.dtype == torch.float64 and got[k].shape == w.shape, k
        if not torch.equal(got[k].view(torch.int64), w.view(torch.int64)):
            differ = got[k].view(torch.int64) != w.view(torch.int64)
            wrong.append((k, int(differ.sum()), got[k][differ][:3].tolist(), w[differ][:3].tolist()))
    assert not wrong, wrong
