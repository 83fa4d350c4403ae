"""CPU: bench.py's command line and its --dump-outputs writer (no device work): a plain run switches every secondary
leg off and --full leaves each at its default; the dump holds float32 verdicts and randomness of the rows it names, the
same rows on every call, under 64 MB in all."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_main", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_has_no_secondary_legs(bench, monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert (a.roofline_steps, a.single_call_steps, a.single_beacon_reps, a.strong_total_rounds) == (0, 0, 0, 0)
    assert a.no_cpu_baseline is True
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.steps == 200
    assert (a.roofline_steps, a.single_call_steps, a.single_beacon_reps, a.strong_total_rounds) == (2, 4, 20, 1 << 20)
    assert a.no_cpu_baseline is False
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--roofline-steps", "0", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.roofline_steps == 0 and a.no_cpu_baseline is True and a.single_call_steps == 4
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.parametrize("n,world,rank", [(1000, 1, 0), (300001, 1, 0), (200000, 2, 1)])
def test_dump_outputs(bench, tmp_path, n, world, rank):
    g = torch.Generator().manual_seed(n)
    verdict = torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g)
    rand = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    tag = "_rank%d" % rank if rank else ""
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), verdict, rand, rank, world)
        assert sorted(os.listdir(tmp_path / d)) == sorted(x + tag + ".npy" for x in ("randomness", "rows", "verdict"))
        got.append({x: np.load(tmp_path / d / (x + tag + ".npy")) for x in ("randomness", "rows", "verdict")})
    a, b = got
    for x in a:
        assert np.array_equal(a[x], b[x])
    want = min(n, (1 << 18) // world)
    rows = a["rows"].astype(np.int64)
    assert a["rows"].dtype == np.float64 and rows.shape == (want,)
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    assert a["verdict"].dtype == np.float32 and np.array_equal(a["verdict"], verdict.numpy()[rows])
    assert a["randomness"].dtype == np.float32 and np.array_equal(a["randomness"], rand.numpy()[rows])
    assert world * sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
