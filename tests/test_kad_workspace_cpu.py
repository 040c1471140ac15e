"""The workspace sizes of the Kernel Audio Distance family are those recorded in tests/golden/kad_workspace.json
(tests/golden/make_goldens_kad.py): every am_*_workspace_bytes of the select, rbf, multi, rows and groups calls, f32 and f64,
on a grid of shapes.  A size is the sum of the norms and of the partials the grid plan and the chunk rules ask for, so a rule
that drifts shows here without a GPU - on the device it would change the summation order and with it the bits."""
import json

import pytest

import make_goldens_kad as rec


@pytest.fixture(scope="module")
def lib():
    import audio_metrics_amd
    return audio_metrics_amd._lib.load()


def test_workspace_sizes_are_the_recorded_ones(lib):
    with open(rec.WORKSPACE_JSON) as f:
        want = json.load(f)
    queries = rec.workspace_queries()
    assert sorted(want) == sorted(name for name, _ in queries)
    for name, args in queries:
        assert len(want[name]) == len(args) and any(v > 0 for v in want[name]), name
        got = [int(getattr(lib, name)(*a)) for a in args]
        wrong = [(a, g, w) for a, g, w in zip(args, got, want[name]) if g != w]
        assert not wrong, (name, len(wrong), wrong[:5])
