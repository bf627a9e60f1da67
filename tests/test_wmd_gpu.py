"""The WMD kernels (csrc/wmd.hip) against numpy and the assignment oracle.

``distances``: against the numpy difference form on float64 casts, entry by entry under
(dim + 4) 2^-52 c -- both sides add dim squares (each to half an ulp of the partial sum) and
take one correctly rounded square root, which halves the relative error of the sum; identical
rows give exactly 0.0.  ``emd_uniform``: against the oracle of tests/wmd_cases.py fed the
device's own D, under that module's bound.  ``emd_uniform`` raises on any non-zero solver
status, so every value checked here came with status 0.  Everything else is bit for bit: a
problem alone, in a batch, in the reversed batch, on any grid and on either capacity instance.
"""
import functools

import numpy as np
import pytest
import torch

from gfedntm_amd.eval import metrics
from gfedntm_amd.ops import wmd
from tests import wmd_cases as cases

pytestmark = pytest.mark.gpu

EPS = cases.EPS


def _bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64),
                          np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dim", [1, 63, 300])
def test_distances(dim, dtype):
    rng = np.random.default_rng(dim)
    Ua, Ub = 70, 130                                  # more than one tile each way, ragged
    a = torch.from_numpy(rng.standard_normal((Ua, dim))).to(dtype)
    b = torch.from_numpy(rng.standard_normal((Ub, dim))).to(dtype)
    b[:40] = a[:40]
    got = wmd.distances(a.cuda(), b.cuda())
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (Ua, Ub)
    got = got.cpu().numpy()
    a64, b64 = a.double().numpy(), b.double().numpy()
    ref = np.sqrt(((a64[:, None, :] - b64[None, :, :]) ** 2).sum(-1))
    err = np.abs(got - ref)
    print(f"dim {dim} {dtype}: worst error / bound {(err / np.maximum((dim + 4) * EPS * ref, 1e-300)).max():.3f}")
    assert (err <= (dim + 4) * EPS * ref).all()
    assert (got[:40].diagonal() == 0.0).all() and (got[40:, 40:] > 0).all()
    # the grid, a row-strided view and the host engine's dtype rule change nothing
    assert _bits(wmd.distances(a.cuda(), b.cuda(), max_grid=1).cpu().numpy(), got)
    wide = torch.zeros(Ua, dim + 3, dtype=dtype, device="cuda")
    wide[:, :dim] = a.cuda()
    assert _bits(wmd.distances(wide[:, :dim], b.cuda()).cpu().numpy(), got)
    assert _bits(wmd.distances(a.double().cuda(), b.cuda()).cpu().numpy(), got)   # widening is exact


@functools.lru_cache(maxsize=None)
def _case(n, m):
    """The device's own D of a shape (on the device and on the host) and the oracle's value."""
    va, vb = cases.vectors(n, m)
    d = wmd.distances(torch.tensor(va, device="cuda"), torch.tensor(vb, device="cuda"))
    h = d.cpu().numpy()
    h.setflags(write=False)
    return d, h, cases.oracle(h)


@pytest.mark.parametrize("n,m", cases.SHAPES)
def test_emd_matches_the_oracle(n, m):
    d, h, ref = _case(n, m)
    assert (h[:min(n, m) // 2].diagonal() == 0.0).all()
    got = wmd.emd_uniform(d, [range(n)], [range(m)])          # (a CUDA dist: the device engine)
    assert got.shape == (1, 1) and got.dtype == np.float64
    print(f"{n} x {m}: |device - oracle| = {abs(got[0, 0] - ref):.3e}, bound {cases.bound(h):.3e}")
    assert abs(got[0, 0] - ref) <= cases.bound(h)
    assert _bits(wmd.emd_uniform(h, [range(n)], [range(m)], engine="device"), got)   # uploaded D


def test_integer_costs_are_exact():
    ints = cases.integer_cases()
    D, la, lb = cases.stacked([c for c, _, _ in ints])
    got = wmd.emd_uniform(torch.from_numpy(D).cuda(), la, lb)      # 200 x 200 problems, ties everywhere
    assert got.shape == (200, 200) and np.isfinite(got).all()
    for k, (_, total, T) in enumerate(ints):
        assert got[k, k] == total / T, k


@functools.lru_cache(maxsize=None)
def _mixed():
    """One table of every shape's words, its D, and the lists of a batch that mixes every shape
    (all cross pairs included) with an empty list on either side."""
    vecs, la, lb, at = [], [], [], 0
    for n, m in cases.SHAPES:
        va, vb = cases.vectors(n, m)
        vecs += [va, vb]
        la.append(list(range(at, at + n)))
        lb.append(list(range(at + n, at + n + m)))
        at += n + m
    table = torch.from_numpy(np.concatenate(vecs)).cuda()
    return wmd.distances(table, table), la + [[]], lb + [[]]


def test_mixed_batch_empty_lists_and_order():
    d, la, lb = _mixed()
    got = wmd.emd_uniform(d, la, lb)
    k = len(cases.SHAPES)
    assert got.shape == (k + 1, k + 1)
    assert np.isinf(got[k]).all() and np.isinf(got[:, k]).all() and np.isfinite(got[:k, :k]).all()
    for i, (n, m) in enumerate(cases.SHAPES):
        alone = wmd.emd_uniform(d, [la[i]], [lb[i]])
        assert _bits(alone, got[i:i + 1, i:i + 1]), (n, m)
        # (the same words as _case: against the oracle once more, through the index lists)
        assert abs(got[i, i] - _case(n, m)[2]) <= cases.bound(_case(n, m)[1])
    rev = wmd.emd_uniform(d, la[::-1], lb[::-1])
    assert _bits(rev[::-1, ::-1], got)


@functools.lru_cache(maxsize=None)
def _forty():
    rng = np.random.default_rng(40)
    table = rng.standard_normal((120, 16))
    la = [rng.choice(120, size=int(s), replace=False).tolist() for s in rng.integers(1, 41, 8)]
    lb = [rng.choice(120, size=int(s), replace=False).tolist() for s in rng.integers(1, 41, 5)]
    t = torch.from_numpy(table).cuda()
    return wmd.distances(t, t), la, lb


@pytest.mark.parametrize("max_grid", [1, 3])
def test_grid_does_not_change_a_bit(max_grid):
    # 40 problems on 4 / 12 waves: every flow slot and LDS slice serves about 10 / 3 of them
    d, la, lb = _forty()
    want = wmd.emd_uniform(d, la, lb)
    assert want.shape == (8, 5) and np.isfinite(want).all()
    assert _bits(wmd.emd_uniform(d, la, lb, max_grid=max_grid), want)
    eye = torch.eye(120, dtype=torch.float64, device="cuda")     # costs 0 and sqrt(2) only: ties
    assert _bits(wmd.pairwise_wmd(la, lb, eye, max_grid=max_grid), wmd.pairwise_wmd(la, lb, eye))


def test_capacity_instances_agree():
    d, la, lb = _forty()
    small = wmd.emd_uniform(d, la[:2], lb[:2], capacity=128)
    large = wmd.emd_uniform(d, la[:2], lb[:2], capacity=512)
    assert _bits(small, large) and _bits(small, wmd.emd_uniform(d, la, lb)[:2, :2])
    with pytest.raises(ValueError, match="capacity"):
        wmd.emd_uniform(_case(130, 130)[0], [range(130)], [range(130)], capacity=128)


def test_mean_min_wmd_device_matches_host():
    rng = np.random.default_rng(5)
    words = [f"w{i}" for i in range(60)]
    dim, nw = 20, 12
    v = rng.standard_normal((60, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    vec = dict(zip(words, v))
    ref = [list(rng.permutation(words + ["oov"])[:14]) for _ in range(4)]
    cmp_ = [list(rng.permutation(words + ["oov"])[:14]) for _ in range(5)] + [["oov"]]
    host = metrics.mean_min_wmd(ref, cmp_, vec, nw, engine="host")
    dev = metrics.mean_min_wmd(ref, cmp_, vec, nw, engine="device")
    # a value is a convex combination of costs <= 2 (unit vectors): the two D differ by
    # (dim + 4) 2^-52 c per entry, the two solvers by the rounding of their sums
    bound = ((2 * nw * nw + 4) + (dim + 4)) * EPS * 2.0
    print(f"mean_min_wmd: |device - host| = {abs(dev - host):.3e}, bound {bound:.3e}")
    assert np.isfinite(host) and abs(dev - host) <= bound
    table = metrics.WordTable(vec, device=True)
    assert table.table.is_cuda
    assert metrics.mean_min_wmd(ref, cmp_, table, nw, engine="device") == dev   # one upload, same bits
    assert abs(metrics.word_movers_distance(ref[0], cmp_[0], vec, engine="device") -
               metrics.word_movers_distance(ref[0], cmp_[0], vec, engine="host")) <= bound


def test_rejected_inputs():
    d = torch.ones(600, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="at most 512"):
        wmd.emd_uniform(d, [range(513)], [[0, 1]])
    assert wmd.emd_uniform(d, [range(512)], [[0, 1]])[0, 0] == 1.0
    for bad in (-1.0, float("nan"), float("inf")):
        e = d.clone()
        e[5, 1] = bad
        with pytest.raises(ValueError, match="finite and non-negative"):
            wmd.emd_uniform(e, [[0, 1]], [[2, 3]])
    with pytest.raises(ValueError, match="outside"):
        wmd.emd_uniform(d, [[0, 600]], [[1]])
    with pytest.raises(ValueError, match="max_grid"):
        wmd.emd_uniform(d, [[0]], [[1]], max_grid=0)
