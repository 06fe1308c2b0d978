"""bench.py command line: --full / --dump-outputs parsing and the output
dump (float32 .npy files, the same seeded parameter positions every run,
bounded size). The benchmark itself is not started here."""
import importlib.util
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _FakeCompiled:
    def __init__(self, named):
        self._named = named

    def named_parameters(self):
        return dict(self._named)


def _params(seed, n_small=7, n_big=3 * 4096 + 5):
    g = torch.Generator().manual_seed(seed)
    return {"small": torch.randn(n_small, generator=g),
            "big": torch.randn(n_big, generator=g).to(torch.bfloat16),
            "mat": torch.randn(130, 70, generator=g)}


def test_args_defaults_and_flags(bench):
    a = bench._parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (4, 2, False, None)
    a = bench._parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"
    with pytest.raises(SystemExit):
        bench._parse_args(["--steps", "0"])


def test_dump_outputs_files(bench, tmp_path):
    named = _params(0)
    loss = torch.tensor(3.25, dtype=torch.bfloat16)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench._dump_outputs(d1, loss, _FakeCompiled(named), rank=0)
    bench._dump_outputs(d2, loss, _FakeCompiled(named), rank=0)
    assert sorted(os.listdir(d1)) == ["loss.npy", "params_sample.npy"]
    l1 = np.load(os.path.join(d1, "loss.npy"))
    s1 = np.load(os.path.join(d1, "params_sample.npy"))
    s2 = np.load(os.path.join(d2, "params_sample.npy"))
    assert l1.dtype == np.float32 and float(l1) == 3.25
    assert s1.dtype == np.float32
    # small tensors whole, large ones sampled
    n = bench._DUMP_PER_PARAM
    assert s1.shape == (7 + n + n,)
    np.testing.assert_array_equal(s1[:7], named["small"].numpy())
    # same positions every run -> identical dumps for identical state
    np.testing.assert_array_equal(s1, s2)
    # ... and a changed parameter shows up at those positions
    changed = dict(named, mat=named["mat"] + 1.0)
    d3 = str(tmp_path / "c")
    bench._dump_outputs(d3, loss, _FakeCompiled(changed), rank=0)
    s3 = np.load(os.path.join(d3, "params_sample.npy"))
    np.testing.assert_array_equal(s3[:7 + n], s1[:7 + n])
    np.testing.assert_allclose(s3[7 + n:], s1[7 + n:] + 1.0, rtol=0,
                               atol=1e-6)


def test_dump_outputs_size_cap_and_ranks(bench, tmp_path):
    # many tensors: the per-tensor sample shrinks so the total stays
    # under 64 MB of float32
    many = {f"p{i}": torch.zeros(8) for i in range(64)}
    old = bench._DUMP_MAX_ELEMS
    bench._DUMP_MAX_ELEMS = 128
    try:
        d = str(tmp_path / "cap")
        bench._dump_outputs(d, torch.tensor(0.0), _FakeCompiled(many), 0)
        s = np.load(os.path.join(d, "params_sample.npy"))
        assert s.size <= 128
    finally:
        bench._DUMP_MAX_ELEMS = old
    assert (old + 1) * 4 <= 64 * 1024 * 1024
    # ranks other than 0 take part in the gather but write nothing
    d = str(tmp_path / "r1")
    bench._dump_outputs(d, torch.tensor(0.0), _FakeCompiled(many), 1)
    assert not os.path.exists(d)
