"""What the fused scorer covers (ops.engine.score_covers) next to what runs on it by default
(score_supports), and the federated document-completion perplexity
(federation/runner.py federation_perplexity, LocalFederation.perplexity,
run_distributed(perplexity_completion=), --perplexity_completion) -- all on the CPU."""
import os
import types

import numpy as np
import pytest
import torch

from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.federation.runner import LocalFederation, federation_perplexity
from gfedntm_amd.ops.engine import score_covers, score_supports
from gfedntm_amd.utils.config import load_config


# ---------------------------------------------------------------------------------- coverage
def _stub(backend="fused", model_type="prodLDA", K=50, label_size=0):
    return types.SimpleNamespace(backend=backend, model_type=model_type, n_components=K,
                                 label_size=label_size)


@pytest.mark.parametrize("kw,covers,supported", [
    (dict(), True, True),
    (dict(K=512), True, True),
    (dict(K=513), False, False),
    (dict(backend="torch"), False, False),
    (dict(model_type="LDA"), True, False),
    (dict(model_type="LDA", K=256), True, False),
    (dict(model_type="LDA", K=257), False, False),
    (dict(label_size=5), True, False),
    (dict(label_size=256, K=256), True, False),
    (dict(label_size=5, K=300), False, False),
    (dict(label_size=257), False, False),
    (dict(model_type="LDA", label_size=5), True, False),
    (dict(model_type="LDA", backend="torch"), False, False),
])
def test_score_covers_against_score_supports(kw, covers, supported):
    tm = _stub(**kw)
    assert score_covers(tm) is covers and score_supports(tm) is supported
    assert covers or not supported                      # the default is never wider than the coverage
    if not covers:
        with pytest.raises(RuntimeError, match="fused scoring unsupported"):
            score_covers(tm, explain=True)
    else:
        assert score_covers(tm, explain=True)


def test_score_supports_keeps_its_reasons():
    with pytest.raises(RuntimeError, match="NeuralLDA"):
        score_supports(_stub(model_type="LDA"), explain=True)
    with pytest.raises(RuntimeError, match="label-head"):
        score_supports(_stub(label_size=3), explain=True)


# ---------------------------------------------------------------------------------- federation
def _params(**kw):
    p = dict(load_config().training_params)
    p.update(num_epochs=2, batch_size=16, hidden_sizes=(16, 16), n_components=5, model_type="LDA")
    p.update(kw)
    return p


def _corpora(n=3, seed=1):
    sc = generate_synthetic(vocab_size=120, n_topics=5, n_docs=40, n_nodes=n, frozen_topics=2,
                            nwords=(15, 30), seed=seed)
    return [ClientCorpus(synthetic=sc, node=i) for i in range(n)]


def _by_hand(tm, datasets, ids, completion, n_samples, seed):
    """The definition, from per-client ``tm.score``: float64 sums of the fp32 RL rows in
    document order, clients in id order."""
    rl_sum, held, obs, n_docs = 0.0, 0, 0, 0
    for c, ds in sorted(zip(ids, datasets), key=lambda t: t[0]):
        r = tm.score(ds, n_samples=n_samples, seed=seed + c, completion=completion)
        part = 0.0
        for v in r["rl"]:
            assert v.dtype == np.float32
            part += float(v)
        rl_sum += part
        held, obs, n_docs = held + r["tokens_heldout"], obs + r["tokens_observed"], n_docs + len(r["rl"])
    return {"perplexity": float(np.exp(rl_sum / held)), "rl_sum": rl_sum, "tokens_heldout": held,
            "tokens_observed": obs, "n_docs": n_docs, "clients": len(ids), "completion": completion,
            "engine": "torch"}


@pytest.mark.parametrize("model_type", ["LDA", "prodLDA"])
def test_federation_perplexity_is_the_per_client_sums(model_type):
    fed = LocalFederation(_corpora(3), _params(model_type=model_type), max_iters=4, device="cpu",
                          backend="torch", seed=2)
    fed.run()
    tm = fed.clients[0].tm
    datas, sets = [c.data for c in fed.clients], [c.dataset for c in fed.clients]
    got = federation_perplexity(tm, datas, completion=0.4, n_samples=2, seed=9)
    assert got == _by_hand(tm, sets, [0, 1, 2], float(0.4), 2, 9)
    assert got["engine"] == "torch" and np.isfinite(got["perplexity"]) and got["perplexity"] > 1
    assert got["tokens_heldout"] + got["tokens_observed"] == int(sum(s.csr.sum() for s in sets))
    # client ids key the split and the draws; LocalFederation passes its clients' (1-based)
    ids = [c.id for c in fed.clients]
    assert ids == [1, 2, 3]
    ref = _by_hand(tm, sets, ids, 0.5, 1, 0)
    assert fed.perplexity() == ref
    assert federation_perplexity(tm, datas[::-1], client_ids=ids[::-1]) == ref      # client order, not list order
    assert fed.perplexity(seed=1)["rl_sum"] != ref["rl_sum"]
    assert fed.perplexity(engine="torch") == ref
    with pytest.raises(RuntimeError, match="fused scoring unsupported"):
        fed.perplexity(engine="fused")
    for bad in (0.0, 1.0):
        with pytest.raises(ValueError):
            fed.perplexity(completion=bad)
    with pytest.raises(ValueError):
        federation_perplexity(tm, datas, client_ids=[1, 2])


def _ppl_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gfedntm_amd.federation.runner import run_distributed
        corpus = _corpora(world)[rank]
        out = run_distributed(corpus, _params(), max_iters=4, backend="torch", seed=2,
                              perplexity_completion=0.5)
        plain = run_distributed(corpus, _params(), max_iters=4, backend="torch", seed=2)
        q.put((rank, {k: v for k, v in out.items() if k.startswith("perplexity")},
               sorted(k for k in plain if "perplexity" in k)))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ppl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the same federation in one process
    fed = LocalFederation(_corpora(2), _params(), max_iters=4, device="cpu", backend="torch", seed=2)
    fed.run()
    one = fed.perplexity(completion=0.5, seed=2)
    want = {"perplexity": one["perplexity"], "perplexity_completion": 0.5,
            "perplexity_tokens": one["tokens_heldout"], "perplexity_engine": "torch"}
    assert np.isfinite(one["perplexity"]) and one["clients"] == 2
    for _, got, plain_keys in res:
        assert got == res[0][1] == want
        assert plain_keys == []                         # perplexity_completion=0: no extra keys


# ---------------------------------------------------------------------------------- CLI
def test_cli_perplexity(tmp_path, capsys):
    from gfedntm_amd.cli import main
    base = ["--workdir", str(tmp_path), "--min_clients_federation", "2", "--max_iters", "4",
            "--engine", "torch", "--device", "cpu", "--generate_synthetic", str(tmp_path / "syn.npz")]
    with pytest.raises(SystemExit):
        main(base + ["--perplexity_completion", "0.5", "--backend", "grpc"])
    with pytest.raises(SystemExit):
        main(base + ["--perplexity_completion", "1.0"])
    capsys.readouterr()
    out = main(base + ["--perplexity_completion", "0.5"])
    logged = capsys.readouterr().out            # (the server logger writes to stdout and a file)
    assert out["rounds"] == 4 and out["perplexity_completion"] == 0.5
    assert np.isfinite(out["perplexity"]) and out["perplexity"] > 1 and out["perplexity_tokens"] > 0
    assert out["perplexity_engine"] == "torch"
    assert "-- -- Global completion perplexity@0.50: " in logged
    assert not any("perplexity" in k for k in main(base))


def test_perplexity_passes_the_engine_on():
    torch.manual_seed(0)
    from gfedntm_amd.data.bow import BOWDataset
    from gfedntm_amd.models import AVITM
    from tests.helpers import random_csr
    X = random_csr(40, 200, 20, seed=1)
    tm = AVITM(input_size=200, n_components=6, model_type="LDA", hidden_sizes=(16, 12), batch_size=16,
               verbose=False, device="cpu", backend="torch")
    ds = BOWDataset(X, {i: str(i) for i in range(200)})
    assert tm.perplexity(ds, seed=3, engine="torch") == tm.perplexity(ds, seed=3)
    with pytest.raises(RuntimeError, match="fused scoring unsupported"):
        tm.perplexity(ds, seed=3, engine="fused")
