"""The exact transport solver behind the batched WMD engines: the numpy twin ("host") of
csrc/wmd.hip against the assignment oracle, and the ``engine`` keyword through eval/metrics.py
and experiments/wmd_eval.py.  The kernels themselves: tests/test_wmd_gpu.py.

Oracle and bound: tests/wmd_cases.py.  Against the default LP path the tolerance is 1e-7, the
default feasibility / optimality tolerances of HiGHS.
"""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

from gfedntm_amd.eval import metrics
from gfedntm_amd.experiments import wmd_eval
from gfedntm_amd.ops import wmd
from tests import wmd_cases as cases


def _solve(c):
    return float(wmd.emd_uniform(c, [range(c.shape[0])], [range(c.shape[1])], engine="host")[0, 0])


@pytest.mark.parametrize("n,m", cases.CPU_SHAPES)
def test_host_twin_matches_the_oracle(n, m):
    va, vb = cases.vectors(n, m)
    c = wmd.distances(va, vb, engine="host")
    assert c.dtype == np.float64 and c.shape == (n, m)
    assert (c[:min(n, m) // 2].diagonal() == 0.0).all()          # shared words cost exactly 0
    got, ref = _solve(c), cases.oracle(c)
    print(f"{n} x {m}: |twin - oracle| = {abs(got - ref):.3e}, bound {cases.bound(c):.3e}")
    assert abs(got - ref) <= cases.bound(c)
    whole = wmd.pairwise_wmd([range(n)], [range(n, n + m)], np.concatenate([va, vb]), engine="host")
    assert whole.shape == (1, 1) and whole[0, 0] == got


def test_integer_costs_are_exact():
    # potentials stay exact on integer costs, and both sides divide the same integer by T once
    for c, total, T in cases.integer_cases():
        assert _solve(c) == total / T, c


def test_equal_costs_and_identical_lists():
    # c k is exact in float64 for these c and every k <= T, so the sum of x_ij c is c T exactly
    for c in (1.0, 0.75, 3.0, 2.0 ** -20):
        for n, m in [(1, 1), (2, 3), (7, 5), (6, 4)]:
            assert _solve(np.full((n, m), c)) == c
    rng = np.random.default_rng(3)
    v = rng.standard_normal((9, 6))
    got = wmd.pairwise_wmd([range(9), [4, 2, 7]], [range(9), [7, 4, 2]], v, engine="host")
    assert got[0, 0] == 0.0 and got[1, 1] == 0.0 and got[0, 1] > 0.0


def _vec(words, dim=5, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((len(words), dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return dict(zip(words, v))


WORDS = [f"w{i}" for i in range(14)]


def test_host_engine_matches_the_lp():
    vec = _vec(WORDS)
    for a, b in [(WORDS[:3], WORDS[2:7]), (WORDS[:6], WORDS[4:10]), (WORDS[5:12], WORDS[:4])]:
        lp = metrics.word_movers_distance(a, b, vec)
        assert metrics.word_movers_distance(a, b, vec, engine="lp") == lp
        assert abs(metrics.word_movers_distance(a, b, vec, engine="host") - lp) <= 1e-7


def test_mean_min_wmd_host_matches_the_default():
    vec = _vec(WORDS)
    ref = [WORDS[:5], ["unknown1"] + WORDS[3:8], WORDS[6:11]]
    cmp_ = [WORDS[2:7], WORDS[8:13] + ["unknown2"], ["unknown1", "unknown2"]]    # one with no vector
    want = metrics.mean_min_wmd(ref, cmp_, vec, 5)
    assert np.isfinite(want)
    assert abs(metrics.mean_min_wmd(ref, cmp_, vec, 5, engine="host") - want) <= 1e-7
    table = metrics.WordTable(vec)
    assert metrics.mean_min_wmd(ref, cmp_, table, 5, engine="host") == \
        metrics.mean_min_wmd(ref, cmp_, vec, 5, engine="host")
    # a reference topic without any known word is at distance inf of everything
    assert metrics.mean_min_wmd([["unknown1"]], cmp_, vec, 5) == float("inf")
    assert metrics.mean_min_wmd([["unknown1"]], cmp_, vec, 5, engine="host") == float("inf")
    assert metrics.word_movers_distance(["unknown1"], WORDS[:2], vec, engine="host") == float("inf")


def _model_folders(root):
    rng = np.random.default_rng(11)
    names = ["non_collaborative_bio_3_0_x", "non_collaborative_cs_3_0_x", "centralized_3_0_x",
             "centralized_5_0_x"]
    for name in names:
        k = int(name.split("_")[-3])
        os.makedirs(os.path.join(root, name))
        with open(os.path.join(root, name, "topics.json"), "w") as f:
            json.dump([[str(w) for w in rng.permutation(WORDS + ["oov"])[:6]] for _ in range(k)], f)


def test_wmd_tables_engine_and_cli(tmp_path):
    _model_folders(str(tmp_path / "models"))
    vec = _vec(WORDS, seed=2)
    np.savez(tmp_path / "vec.npz", words=np.array(WORDS), vectors=np.stack([vec[w] for w in WORDS]))
    vectors = wmd_eval.load_vectors(str(tmp_path / "vec.npz"))
    want = wmd_eval.wmd_tables(str(tmp_path / "models"), str(tmp_path / "lp"), vectors, [3], [4, 6])
    got = wmd_eval.wmd_tables(str(tmp_path / "models"), str(tmp_path / "host"), vectors, [3], [4, 6],
                              engine="host")
    cli = wmd_eval.main(["--path_models", str(tmp_path / "models"), "--path_save", str(tmp_path / "cli"),
                         "--vectors", str(tmp_path / "vec.npz"), "--nr_tpcs_lst", "3",
                         "--n_words_lst", "4,6", "--engine", "host"])
    assert len(want) == len(got) == len(cli) == 2
    for w, g, c in zip(want, got, cli):
        tw, tg, tc = (pd.read_csv(f, index_col=0) for f in (w, g, c))
        assert os.path.basename(w) == os.path.basename(g) == os.path.basename(c)
        assert tw.shape == (2, 4) and list(tw.columns) == list(tg.columns) == list(tc.columns)
        assert list(tw.index) == list(tg.index)
        assert np.abs(tw.to_numpy() - tg.to_numpy()).max() <= 1e-7
        assert np.array_equal(tg.to_numpy(), tc.to_numpy())


def test_rejected_inputs():
    vec = _vec(WORDS)
    d = np.ones((4, 4))
    for call in (lambda: metrics.word_movers_distance(WORDS[:2], WORDS[2:4], vec, engine="fused"),
                 lambda: metrics.mean_min_wmd([WORDS[:2]], [WORDS[2:4]], vec, engine="gpu"),
                 lambda: wmd_eval.wmd_tables("nowhere", "nowhere", vec, engine="fast"),
                 lambda: wmd.emd_uniform(d, [[0]], [[1]], engine="lp"),
                 lambda: wmd.distances(d, d, engine="lp")):
        with pytest.raises(ValueError, match="engine"):
            call()
    big = np.ones((wmd.max_words() + 1, 2))
    assert wmd.max_words() == 512
    with pytest.raises(ValueError, match="at most 512"):
        wmd.emd_uniform(big, [range(513)], [[0, 1]], engine="host")
    with pytest.raises(ValueError, match="at most 512"):
        wmd.pairwise_wmd([[0]], [[0] * 513], np.ones((3, 2)), engine="host")
    for bad in (-1.0, float("nan"), float("inf")):
        e = d.copy()
        e[2, 1] = bad
        with pytest.raises(ValueError, match="finite and non-negative"):
            wmd.emd_uniform(e, [[0, 1]], [[2, 3]], engine="host")
    with pytest.raises(ValueError, match="outside"):
        wmd.emd_uniform(d, [[0, 4]], [[1]], engine="host")
    with pytest.raises(ValueError, match="max_grid"):
        wmd.emd_uniform(d, [[0]], [[1]], engine="host", max_grid=0)


def test_device_engine_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    d = np.ones((2, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        wmd.emd_uniform(d, [[0]], [[1]], engine="device")
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.mean_min_wmd([["w0"]], [["w1"]], _vec(WORDS), engine="device")
