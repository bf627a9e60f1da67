"""Where a run of rounds per graph replay ends (runner.round_cuts / host_after_round /
run_plan), and the per-step epoch index the step kernels get (data.bow.epoch_index).

With the epoch loss sums kept on the device an epoch end is no host access: runs are not cut
there and ``more`` holds across it.  Heavy rounds, the warmup end, the poll, digest, metrics
and checkpoint boundaries and the last round still cut a run and clear ``more``.  With the
sums on the host the cuts are the ones the round loops made before the functions were factored
out of them (re-derived here from that definition)."""
import numpy as np
import pytest

from gfedntm_amd.data.bow import BatchPlan, epoch_index
from gfedntm_amd.federation.runner import host_after_round, round_cuts, run_plan


def _walk(n_rounds, kmax, ends, **every):
    """[(first round, k, more)] of a whole run, as the round loops drive run_plan."""
    out, it = [], 0
    while it < n_rounds:
        k, more = run_plan(it, kmax, ends, **every)
        out.append((it, k, more))
        it += k
    return out


def _covers(replays, r):
    return next((it, k, more) for it, k, more in replays if it <= r < it + k)


N, KMAX = 100, 16
EPOCH_ENDS = list(range(4, N, 5))          # 5-step epochs


def test_device_sums_runs_span_epoch_ends():
    ends = round_cuts(EPOCH_ENDS, heavy=[], last=N - 1, device_sums=True)
    assert ends == {N - 1}
    replays = _walk(N, KMAX, ends)
    # whole kmax-round replays, each spanning epoch ends, chained by ``more``
    assert replays[0] == (0, 16, True)
    assert all(k == 16 and more for _, k, more in replays[:6])
    for e in EPOCH_ENDS[:-1]:
        it, k, more = _covers(replays, e)
        assert not host_after_round(e, ends)
        assert it + k - 1 != e or more          # an epoch end closing a replay keeps ``more``
    assert sum(k for _, k, _ in replays) == N
    assert replays[-1][2] is False              # the last round


@pytest.mark.parametrize("what", ["heavy", "warmup", "poll", "digest", "metrics", "checkpoint", "last"])
def test_device_sums_remaining_cuts(what):
    r = 36                                      # (37 rounds: the boundaries' period)
    kw = dict(heavy=[], last=N - 1, device_sums=True)
    every = {}
    if what == "heavy":
        kw["heavy"] = [r]
    elif what == "warmup":
        kw["warmup_end"] = r
    elif what == "last":
        kw["last"] = r
    else:
        every = {what + "_every": r + 1}
    ends = round_cuts(EPOCH_ENDS, **kw)
    assert host_after_round(r, ends, **every)
    replays = _walk(kw["last"] + 1, KMAX, ends, **every)
    it, k, more = _covers(replays, r)
    assert it + k - 1 == r and more is False    # the run ends at r and nothing chains on
    # and no replay starts before r and passes it
    assert all(not (i <= r < i + kk - 1) for i, kk, _ in replays)
    # the round before it does not cut (37 is no epoch end and no other boundary)
    assert not host_after_round(r - 1, ends, **every)


def test_host_sums_are_the_parents_cuts():
    heavy, last, warm = [49], N - 1, 9
    ends = round_cuts(EPOCH_ENDS, heavy, last, warm, device_sums=False)
    assert ends == set(EPOCH_ENDS) | {49, N - 1, 9}
    every = dict(poll_every=32, digest_every=32, metrics_every=0, checkpoint_every=25)

    # the definition the round loop carried inline before
    def host_after(r):
        n1 = r + 1
        return bool(r in ends or n1 % 32 == 0 or n1 % 25 == 0)

    def run_end(it):
        r = it
        while r < it + KMAX - 1 and not host_after(r):
            r += 1
        return r

    it = 0
    while it < N:
        k = 1 << ((run_end(it) - it + 1).bit_length() - 1)
        more = not host_after(it + k - 1)
        assert run_plan(it, KMAX, ends, **every) == (k, more)
        assert k <= 4 or it + k - 1 in ends     # 5-step epochs: no replay passes an epoch end
        it += k
    for r in range(N):
        assert host_after_round(r, ends, **every) == host_after(r)


def test_one_round_per_replay_never_chains():
    assert run_plan(3, 1, {99}) == (1, False)


@pytest.mark.parametrize("n_docs,batch,n_steps", [(37, 8, 15), (37, 8, 13), (53, 8, 15), (64, 64, 7),
                                                  (40, 8, 1)])
def test_epoch_index_matches_epoch_end(n_docs, batch, n_steps):
    plan = BatchPlan.build(n_docs, batch, n_steps, seed=3)
    idx = epoch_index(plan.epoch_end)
    assert idx.dtype == np.int32 and idx.shape == (n_steps,)
    e = 0
    for s in range(n_steps):
        assert idx[s] == e
        starts = s == 0 or idx[s - 1] != idx[s]
        assert starts == (s == 0 or bool(plan.epoch_end[s - 1]))
        if plan.epoch_end[s]:
            e += 1
    np.testing.assert_array_equal(idx, plan.epoch)
    # a plan whose last epoch is incomplete still has a slot for it
    per_epoch = -(-n_docs // batch)
    assert int(idx[-1]) + 1 == -(-n_steps // per_epoch)
    if n_steps % per_epoch:
        assert not plan.epoch_end[-1]
