"""bench.py --dump-outputs: what the timed loop's last step returned, written as DIR/<name>.npy (float64, at most 64 MB in all),
from seeded inputs that are the same on every run -- so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    arrays = {"loglik": np.array([-1.5]), "csd_pred": np.arange(24.0).reshape(2, 3, 4), "grad": np.ones((3, 2), dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["csd_pred.npy", "grad.npy", "loglik.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)


def test_large_outputs_are_sampled_to_the_limit_the_same_way_every_time(tmp_path):
    n = bench.DUMP_LIMIT_BYTES // 8
    arrays = {"loglik": np.array([3.25]), "csd_pred": np.arange(float(n)).reshape(-1, 100),
              "csd_pred_list": -np.arange(float(n // 2))}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
        assert _sizes(tmp_path / d) <= bench.DUMP_LIMIT_BYTES
    assert np.load(tmp_path / "a" / "loglik.npy").tolist() == [3.25]
    for name in ("csd_pred", "csd_pred_list"):
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("a", "b"))
        assert a.dtype == np.float64 and np.array_equal(a, b)
        flat = np.abs(a)                                     # (the values are the flat indices they were taken from)
        assert 0.3 * arrays[name].size < a.size < arrays[name].size and np.all(np.diff(flat) > 0)
        assert np.array_equal(arrays[name].reshape(-1)[flat.astype(np.int64)], a)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--workload", "potrf", "--dump-outputs", "x"]])
def test_arguments_without_a_timed_step_to_dump_or_divide_by_are_refused(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.gpu
def test_dumped_outputs_are_the_timed_steps_results_on_the_regenerated_inputs(tmp_path):
    """The dump of a short cfg2 run against the oracle on inputs drawn again here: the log-likelihood and the posterior mean
    with its per-component list are what the timed step computed, and the inputs are the ones bench.py used."""
    from oracle import gpcsd_oracle as O
    R = 6
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--trials-per-gpu", str(R), "--steps", "3",
           "--warmup", "1", "--setup-steps", "3", "--only-value", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    w = bench.workload("cfg2")
    m = bench.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
    lfp = bench.synth_data(w, m, R, seed=1000)
    _, geom, hp, hp0 = bench.oracle_setup(w, m)
    ll = np.load(tmp_path / "loglik.npy")
    assert ll.shape == (1,) and ll[0] == rec["loglik"]
    ll_ref = O.loglik(geom, hp, lfp)
    assert abs(ll[0] - ll_ref) <= 1e-9 * abs(ll_ref)
    ref = O.predict(geom, hp0, lfp, w["x"], w["t"], type="csd")
    csd, csd_list = np.load(tmp_path / "csd_pred.npy"), np.load(tmp_path / "csd_pred_list.npy")
    assert csd.shape == (24, 500, R) and csd_list.shape == (2, 24, 500, R)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert rel(csd, ref["csd"]) < 1e-6 and max(rel(csd_list[i], ref["csd_list"][i]) for i in range(2)) < 1e-6
