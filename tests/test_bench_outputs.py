"""bench.py's plain run, --dump-outputs and --full.

CPU: what --dump-outputs stores for an array (dtype, the size cap, the fixed seeded sample) and
the argument checks. GPU (a 24^3 problem, in process): a plain run prints the headline without
the measurements that moved behind --full, times exactly --steps cycles, and dumps the iterate
those cycles left in x — bit for bit the iterate of warmup + steps cycles from the same x0, and
the same in a second run; --full adds the other lines to the same headline."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
            "warmup", "n_gpus")
FULL_ONLY = ("roofline", "roofline_generic_csr", "fine_spmv_formats", "conv_factor_10cycles",
             "general_rhs", "factored_p0", "pcie_inclusive", "variable_coefficient_c4",
             "cpu_baseline", "cpu_baseline_parallel")


def test_dump_array_small_is_whole():
    import bench
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    d = bench.dump_array(a)
    assert d.dtype == np.float32 and np.array_equal(d, a.ravel())
    d = bench.dump_array(np.arange(5, dtype=np.int32))
    assert d.dtype == np.float64 and np.array_equal(d, np.arange(5.0))
    d = bench.dump_array(np.linspace(0, 1, 7))
    assert d.dtype == np.float64 and np.array_equal(d, np.linspace(0, 1, 7))


def test_dump_array_large_is_a_fixed_sample(monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 800)
    a = np.arange(1000, dtype=np.float64)
    assert np.array_equal(bench.dump_array(a[:100]), a[:100])  # exactly at the cap: whole
    d = bench.dump_array(a)
    assert d.shape == (100,) and d.nbytes <= 800
    assert np.all(np.diff(d) > 0)  # distinct positions in ascending order
    assert np.array_equal(bench.dump_array(a.copy()), d)  # the same positions every time
    assert np.array_equal(bench.dump_array(a * 2.0), d * 2.0)
    f = bench.dump_array(a.astype(np.float32))
    assert f.dtype == np.float32 and f.shape == (200,)


def test_dump_outputs_writes_npy(tmp_path):
    import bench
    assert bench.DUMP_MAX_BYTES * 2 <= 64 << 20
    d = tmp_path / "a" / "b"
    bench.dump_outputs(str(d), {"x": np.arange(4.0), "y": np.ones(3, dtype=np.float32)})
    assert sorted(os.listdir(d)) == ["x.npy", "y.npy"]
    assert np.array_equal(np.load(d / "x.npy"), np.arange(4.0))
    assert np.load(d / "y.npy").dtype == np.float32


@pytest.mark.parametrize("argv", (["--steps", "0"], ["--warmup", "-1"],
                                  ["--gpus", "2", "--dump-outputs", "d"],
                                  ["--dist", "--dump-outputs", "d"]))
def test_bad_arguments_are_refused(argv, capsys):
    import bench
    with pytest.raises(SystemExit) as e:
        bench.main(argv)
    assert e.value.code == 2
    capsys.readouterr()


def _line(capsys):
    rows = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(rows) == 1
    return json.loads(rows[0])


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path, capsys):
    import torch
    import bench
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    n1, steps, warmup = 24, 3, 2
    dumps = []
    for k in range(2):
        d = tmp_path / f"d{k}"
        bench.main(["--gpus", "1", "--n", str(n1), "--steps", str(steps), "--warmup", str(warmup),
                    "--dump-outputs", str(d)])
        out = _line(capsys)
        for key in HEADLINE:
            assert key in out, key
        for key in FULL_ONLY + ("roofline_unstructured_c3",):
            assert key not in out, key
        assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
        assert out["unit"] == "V-cycles/s" and out["dtype"] == "f64" and out["higher_is_better"]
        assert out["ms_per_step"] > 0
        assert abs(out["value"] * out["ms_per_step"] / 1e3 - 1.0) < 1e-2  # the same timing
        assert os.listdir(d) == ["x.npy"]
        dumps.append(np.load(d / "x.npy"))
    n = n1 ** 3
    assert dumps[0].dtype == np.float64 and dumps[0].shape == (n,)
    assert np.array_equal(dumps[0], dumps[1])
    # the same hierarchy and x0 as the bench's, warmup + steps cycles with the history kept
    H = Hierarchy.build(problems.poisson_3d_7pt(n1), alpha=0.1, strength_mode="invabs",
                        max_coarse=2000, aggregation="reference", coarse_order="sorted")
    x0 = np.random.RandomState(0).randn(n)
    x0 /= np.linalg.norm(x0)
    x = torch.as_tensor(x0).cuda()
    hist = H.cycle(torch.zeros(n, dtype=torch.float64, device="cuda"), x, warmup + steps)
    assert len(hist) == warmup + steps and hist[-1] < hist[0]
    assert np.array_equal(dumps[0], x.cpu().numpy())
    assert np.abs(dumps[0]).max() > 0


@pytest.mark.gpu
def test_full_run_adds_the_other_lines(capsys):
    import bench
    bench.main(["--gpus", "1", "--n", "24", "--steps", "3", "--warmup", "1", "--full", "--no-c3",
                "--cpu-cycles", "2", "--cpu-par-cycles", "2"])
    out = _line(capsys)
    for key in HEADLINE + FULL_ONLY:
        assert key in out, key
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert "agree with GPU: True" in out["cpu_baseline"]["sample"]
    assert "agree with GPU: True" in out["cpu_baseline_parallel"]["sample"]
