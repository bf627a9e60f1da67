"""bench.py's command line: a plain run is lean (no side measurements), ``--full`` switches
them on, ``--dump-outputs`` writes the timed rounds' results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--clients", "2", "--docs", "128",
         "--vocab", "400", "--topics", "10", "--nwords", "20,40"]


def test_full_is_off_by_default():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two plain runs with the same arguments and one ``--full`` run of the same small
    federation, side by side (most of a run this small is process start-up):
    name -> (record, {file: array})."""
    tmp = tmp_path_factory.mktemp("bench")
    extra = {"a": [], "b": [], "full": ["--full", "--npmi-steps", "20"]}
    procs = {n: subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + e
                                 + ["--dump-outputs", str(tmp / n)], cwd=ROOT,
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for n, e in extra.items()}
    try:
        outs = {n: p.communicate(timeout=200) for n, p in procs.items()}
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    res = {}
    for n, p in procs.items():
        so, se = outs[n]
        assert p.returncode == 0, se[-3000:]
        d = tmp / n
        res[n] = (json.loads(so.strip().splitlines()[-1]),
                  {f: np.load(d / f) for f in sorted(os.listdir(d))})
    return res


def _headline(rec):
    assert rec["steps"] == 6 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "docs/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(runs):
    """The plain record carries the headline fields and no side measurement, and two runs
    with the same arguments leave the same arrays (same inputs; same build)."""
    (rec, dump), (_, dump_b) = runs["a"], runs["b"]
    _headline(rec)
    assert rec["npmi"] is None and "tss_client1" not in rec
    assert "local_steps_device_ms" not in rec["round_split_ms"]
    assert sorted(dump) == ["client01_loss.npy", "client01_state.npy",
                            "client02_loss.npy", "client02_state.npy"]
    assert sum(x.nbytes for x in dump.values()) <= 64 * 10 ** 6
    for f, x in dump.items():
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), f
        # the same inputs and the same kernels: equal up to the order of atomic sums
        # (fp32 eps 6e-8 times the few thousand terms of a sum)
        np.testing.assert_allclose(dump_b[f], x, rtol=1e-4, atol=1e-6, err_msg=f)
    # the clients end the last round on the same averaged shared state, not on equal losses
    assert dump["client01_loss.npy"][0] != dump["client02_loss.npy"][0]


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements(runs):
    """``--full``: the quality federation and the local-steps replay run after the timed
    rounds, so the record gains their figures and the dumped arrays are those of the
    plain run."""
    (rec, dump), (_, plain) = runs["full"], runs["a"]
    _headline(rec)
    assert np.isfinite(rec["npmi"]) and rec["npmi_rounds"] == 20
    assert np.isfinite(rec["tss_client1"]) and np.isfinite(rec["dss_client1"])
    assert rec["round_split_ms"]["local_steps_device_ms"] > 0
    for f, x in plain.items():
        np.testing.assert_allclose(dump[f], x, rtol=1e-4, atol=1e-6, err_msg=f)
