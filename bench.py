#!/usr/bin/env python
"""Headline benchmark: whole-node docs/s of the 8-client federated ProdLDA K=50.

BASELINE.json metric: "docs/sec (whole node) + NPMI, ProdLDA K=50 8-client fed on
synthetic BoW".  Config (reference config/dft_params.cf defaults + the reference
synthetic generator, src/utils/generate_synthetic.py): V=5000 generator vocabulary,
K=50 topics, hidden (50, 50), softplus, dropout 0.2, Adam(lr 2e-3, betas (0.99, 0.99)),
batch 64 per client, 1000 documents per client of 150-250 tokens, 5 frozen topics.

One *step* = one federation round exactly as the reference defines it
(federated_avitm.py:51-147 + server.py:436-521): every client does one local
minibatch step (forward, backward, Adam) and the sample-weighted average of
all shared tensors (the 20 AVITM state_dict tensors of grads_to_share) replaces
every client's copy.  On MI355X: fused HIP step + the FedAvg all-reduce over
xGMI captured in the same hipGraph (one replay per round).

Default: the 8-client federation of BASELINE.json (``--clients 8``) spread over the N
ranks in contiguous blocks -- all eight clients on one GPU at N = 1 (their steps batched
into one launch per kernel phase, the FedAvg an in-rank fold), four per GPU at N = 2, one
per GPU at N = 8 (the in-step xGMI all-reduce).  The total work per round is fixed
(``scaling: strong``); ``--clients-per-gpu M`` instead fixes M clients per GPU (weak).

``--path runner`` (default) times the PRODUCTION round loop,
:func:`gfedntm_amd.federation.runner.run_distributed` -- what ``main.py
--backend rccl`` users get, with its per-round client bookkeeping.  ``--path engine``
times the bare replay loop of the same engine instead.

``value`` = total training documents of all clients / round time.  Vocabulary
consensus and init broadcast run outside the timed region.

A plain run does only what the headline needs: set up, ``--warmup`` rounds, ``--steps``
timed rounds, the result line.  ``--full`` adds every side measurement, each a run of
its own after the timed rounds: the engine-only replay loop next to the runner's
(``engine_only_ms_per_step``), the round split (the local steps alone / the collective
detached), and the quality numbers -- NPMI (and client 1's TSS / DSS) from a SEPARATE
untimed federation of ``--npmi-steps`` rounds (default 2000), so they do not depend on
``--steps``.

``--dump-outputs DIR`` writes what the timed rounds left behind, after the last of them:
per client ``client<id>_state.npy`` (every float parameter and buffer of its model, the
flat state the round loop updates in place; float32) and ``client<id>_loss.npy`` (the
loss of its last timed step; float64).  An array over its share of 64 MB is cut down to
a fixed, seeded sample of its elements.  The corpus, the initial weights and the
training noise derive from ``--seed``, so two builds run with the same arguments get
the same inputs.

``--sim-clients M`` (one GPU): M simulated clients in one process
(:class:`LocalFederation`: all clients' steps + the in-process FedAvg kernel in
one hipGraph per round) -- a side measurement with its own metric label.

Launch: ``python bench.py`` (1 GPU); ``python bench.py --gpus N`` spawns N ranks
itself (one per GPU) unless it was started by ``torch.distributed.run``
(RANK / WORLD_SIZE in the environment).  ``GFEDNTM_REHEARSE_1GPU=1`` puts every
rank on cuda:0 over gloo (protocol rehearsal on a one-GPU box; timings meaningless).
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Reference numbers (BASELINE.md part B, measured on the unmodified reference):
# 8-client loopback gRPC federation with the built-in sleeps removed.
BASELINE_FED_DOCS_PER_S = 111.0
BASELINE_CPU_CENTRALIZED_DOCS_PER_S = 17300.0
METRIC = "docs/sec (whole node) + NPMI, ProdLDA K=50 8-client fed on synthetic BoW"
# the configuration BASELINE.json's metric is quoted on (reference dft_params.cf defaults +
# the reference generator); only a line of exactly this config carries METRIC / vs_baseline
HEADLINE = {"family": "avitm", "model": "prodLDA", "vocab": 5000, "topics": 50, "hidden": "50,50",
            "batch": 64, "docs": 1000, "nwords": "150,250", "dtype": "fp32", "solver": "adam",
            "backend": "fused", "contextual_size": 768}


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--path", default="runner", choices=["runner", "engine"])
    p.add_argument("--sim-clients", type=int, default=0,
                   help="M > 0: M simulated clients on one GPU (LocalFederation round graph)")
    p.add_argument("--clients", type=int, default=8,
                   help="federated clients in total (BASELINE: 8), spread over the ranks in "
                        "contiguous blocks -- one per GPU at --gpus 8, all eight on one GPU at "
                        "--gpus 1 (total work fixed: strong scaling)")
    p.add_argument("--clients-per-gpu", type=int, default=None,
                   help="instead of --clients: every rank hosts M clients, M x N in total "
                        "(per-GPU work fixed: weak scaling)")
    p.add_argument("--unbatched", action="store_true",
                   help="--sim-clients: one graph branch per client instead of one batched "
                        "launch per phase for all clients (grid z = client)")
    p.add_argument("--serial-clients", action="store_true",
                   help="--sim-clients: capture the clients' steps one after the other "
                        "(default: each client on its own graph branch)")
    p.add_argument("--model", default="prodLDA", choices=["prodLDA", "LDA"])
    p.add_argument("--family", default="avitm", choices=["avitm", "ctm", "zeroshot"],
                   help="ctm = CombinedTM, zeroshot = ZeroShotTM, with --contextual-size "
                        "synthetic embeddings")
    p.add_argument("--contextual-size", type=int, default=768)
    p.add_argument("--vocab", type=int, default=5000)
    p.add_argument("--topics", type=int, default=50)
    p.add_argument("--hidden", default="50,50")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--docs", type=int, default=1000)
    p.add_argument("--nwords", default="150,250", help="document length range [lo, hi)")
    p.add_argument("--backend", default="fused", choices=["fused", "torch"])
    p.add_argument("--allreduce", default=None, choices=[None, "auto", "xgmi", "rccl"],
                   help="FedAvg collective (default: auto = validated xGMI kernel, else RCCL)")
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--npmi-steps", type=int, default=2000,
                   help="rounds of the separate untimed federation the NPMI is computed on "
                        "(0 = skip)")
    p.add_argument("--no-npmi", action="store_true",
                   help="--full without the quality federation")
    p.add_argument("--full", action="store_true",
                   help="also run the side measurements (engine-only loop, round split, "
                        "NPMI / TSS / DSS); a plain run times the rounds and nothing else")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="write the state the timed rounds computed as DIR/<name>.npy")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                   help="decoder GEMM operands (bf16: BASELINE config 'ProdLDA K=50 centralized "
                        "bf16' -- bf16 MFMA operands, fp32 accumulation, fp32 master weights and "
                        "Adam; the headline is fp32, the reference's precision)")
    p.add_argument("--solver", default="adam",
                   choices=["adam", "sgd", "adagrad", "adadelta", "rmsprop"],
                   help="optimizer (reference default adam; the others run in gradient mode)")
    return p.parse_args(argv)


# ---------------------------------------------------------------------------
# process setup
# ---------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawned(local_rank: int, world: int, port: int, argv):
    os.environ.update(RANK=str(local_rank), LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    run(parse(argv))


def _init(args):
    """(rank, world, device, rehearse); initialises the process group (also for one rank,
    so the production runner sees the same control plane at every N)."""
    rehearse = os.environ.get("GFEDNTM_REHEARSE_1GPU") == "1"
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if rehearse else int(os.environ.get("LOCAL_RANK", "0"))
    if "MASTER_PORT" not in os.environ:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
                          RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(local_rank)
    if rehearse:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))
    return rank, world, torch.device("cuda", local_rank), rehearse


# ---------------------------------------------------------------------------
# data / params
# ---------------------------------------------------------------------------
def _corpus(args, n_nodes: int):
    from gfedntm_amd.data.synthetic import generate_synthetic
    lo, hi = (int(x) for x in args.nwords.split(","))
    return generate_synthetic(vocab_size=args.vocab, n_topics=args.topics, n_docs=args.docs,
                              n_nodes=max(n_nodes, 1), frozen_topics=5, nwords=(lo, hi),
                              seed=args.seed)


def _client_corpus(args, sc, node: int):
    from gfedntm_amd.federation.data import ClientCorpus
    emb = None
    if args.family in ("ctm", "zeroshot"):
        # SBERT is not available offline: per-document embeddings are synthetic
        # (a fixed random projection of the document's topic mixture plus noise)
        rng = np.random.default_rng(args.seed + 17 * node)
        proj = np.random.default_rng(args.seed).standard_normal(
            (args.topics, args.contextual_size)).astype(np.float32)
        dt = np.asarray(sc.doc_topics[node], dtype=np.float32)
        emb = dt @ proj + 0.1 * rng.standard_normal(
            (dt.shape[0], args.contextual_size)).astype(np.float32)
    return ClientCorpus(synthetic=sc, node=node, embeddings=emb)


def _params(args):
    from gfedntm_amd.utils.config import load_config
    p = dict(load_config().training_params)
    p.update(n_components=args.topics, model_type=args.model, batch_size=args.batch,
             hidden_sizes=tuple(int(h) for h in args.hidden.split(",")), solver=args.solver,
             contextual_size=args.contextual_size, num_epochs=10 ** 6)
    if args.dtype != "fp32":
        p["matmul_dtype"] = args.dtype
    return p


def _model_type(args) -> str:
    return {"avitm": "avitm", "ctm": "ctm", "zeroshot": "zeroshot"}[args.family]


def _npmi(tm, sc, terms, n_nodes, device) -> float:
    import scipy.sparse as sp
    from gfedntm_amd.data.synthetic import remap_to_vocabulary
    from gfedntm_amd.data.vocab import vocabulary_dict
    from gfedntm_amd.eval.metrics import npmi_coherence
    vocab = vocabulary_dict(terms)
    ref = sp.vstack([remap_to_vocabulary(sc, i, vocab) for i in range(n_nodes)])
    topics_idx = torch.topk(tm.model.beta.detach(), 10, dim=1).indices.cpu().numpy()
    return float(npmi_coherence(topics_idx, ref, device=device))


def _union_terms(sc, n_nodes):
    from gfedntm_amd.data.synthetic import node_vocabulary_terms
    from gfedntm_amd.data.vocab import union_vocabulary
    return union_vocabulary([node_vocabulary_terms(sc, i) for i in range(n_nodes)])


# ---------------------------------------------------------------------------
# outputs of the timed rounds
# ---------------------------------------------------------------------------
DUMP_BUDGET_BYTES = 60 << 20          # all files of a run stay under 64 MB


def _dump_outputs(args, clients, last_step: int, total: int):
    """``--dump-outputs``: the state of this rank's clients after the last timed round
    (call before anything else steps the engines).  ``total`` = clients of the whole
    federation, every one of them gets the same share of the budget."""
    if not args.dump_outputs:
        return
    os.makedirs(args.dump_outputs, exist_ok=True)
    cap = DUMP_BUDGET_BYTES // (4 * max(total, 1))          # float32 elements per client
    torch.cuda.synchronize()
    for c in clients:
        state = c.tm.flat.buffer.detach().float().cpu().numpy().ravel()
        if state.size > cap:
            idx = np.sort(np.random.default_rng(12345).choice(state.size, cap, replace=False))
            state = state[idx]
        np.save(os.path.join(args.dump_outputs, f"client{c.id:02d}_state.npy"), state)
        loss = c.tm.engine.loss_hist[last_step: last_step + 1].detach().cpu().numpy()
        np.save(os.path.join(args.dump_outputs, f"client{c.id:02d}_loss.npy"),
                loss.astype(np.float64))


# ---------------------------------------------------------------------------
# measurements
# ---------------------------------------------------------------------------
def _max_over_ranks(x: float, world: int) -> float:
    if world == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64)
    g = _ctrl_group()
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=g)
    return float(t.item())


_CTRL = None


def _ctrl_group():
    global _CTRL
    if _CTRL is None:
        _CTRL = dist.new_group(backend="gloo") if dist.get_backend() != "gloo" else dist.group.WORLD
    return _CTRL


def _engine_loop(eng, s0: int, s1: int, world: int):
    """Bare replay loop over steps [s0, s1) of an already warmed engine, barrier + device
    sync on both sides: (host wall seconds, device seconds between two events recorded
    around the replays), each the max over ranks."""
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier(group=_ctrl_group())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for s in range(s0, s1):
        eng.step(s)
    ev1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if world > 1:
        dist.barrier(group=_ctrl_group())
    return _max_over_ranks(wall, world), _max_over_ranks(ev0.elapsed_time(ev1) * 1e-3, world)


def _physical_gpus(device, world: int) -> int:
    """Distinct GPUs under the ranks (a one-GPU rehearsal of N ranks is 1)."""
    props = torch.cuda.get_device_properties(device)
    key = (socket.gethostname(), props.pci_domain_id, props.pci_bus_id, props.pci_device_id)
    if world == 1:
        return 1
    keys = [None] * world
    dist.all_gather_object(keys, key, group=_ctrl_group())
    return len(set(keys))


def total_clients(args, world: int) -> int:
    return args.clients_per_gpu * world if args.clients_per_gpu else args.clients


def run_multi(args, rank, world, device, rehearse):
    """A block of clients per rank: the production runner (federation/runner.py
    run_distributed) with federation/rank_round.py MultiClientRound (or the one-client
    round on ranks that host one)."""
    from gfedntm_amd.federation.hierarchical import assign_clients, run_distributed_multi
    physical = _physical_gpus(device, world)
    n_clients = total_clients(args, world)
    sc = _corpus(args, n_clients)
    ids = assign_clients(n_clients, world)[rank]
    corpora = [_client_corpus(args, sc, i - 1) for i in ids]
    kw = dict(backend=args.backend, seed=args.seed, graph=not args.no_graph,
              allreduce=args.allreduce, rehearse_1gpu=rehearse)
    from gfedntm_amd.federation.runner import CommError
    fallback = None
    try:
        out = run_distributed_multi(corpora, ids, _params(args), _model_type(args),
                                    max_iters=args.warmup + args.steps,
                                    timing_warmup=args.warmup, keep_round=True, **kw)
    except CommError as e:
        # the ranks agreed on a data-plane failure (a timed-out xGMI wait or diverged
        # replicas): with auto-selection, measure the same federation over RCCL instead
        if args.allreduce not in (None, "auto"):
            raise
        fallback = f"xGMI all-reduce failed ({e}); re-run over RCCL"
        if rank == 0:
            print(f"[bench] {fallback}", file=sys.stderr, flush=True)
        kw["allreduce"] = "rccl"
        for k in ("GFEDNTM_INJECT_STALL", "GFEDNTM_INJECT_CORRUPT"):
            os.environ.pop(k, None)
        out = run_distributed_multi(corpora, ids, _params(args), _model_type(args),
                                    max_iters=args.warmup + args.steps,
                                    timing_warmup=args.warmup, keep_round=True, **kw)
    wall = _max_over_ranks(out["wall_s"], world)
    dev_s = None if out.get("device_s") is None else _max_over_ranks(out["device_s"], world)
    t = torch.tensor([float(out["docs"])], dtype=torch.float64)
    dist.all_reduce(t, group=_ctrl_group())
    docs = float(t.item())
    eng = out["clients"][0].tm.engine
    n_rounds = args.warmup + args.steps
    final_loss = float(np.mean(eng.loss_hist[max(0, n_rounds - 20): n_rounds].cpu().numpy()))
    _dump_outputs(args, out["clients"], n_rounds - 1, n_clients)
    # round split (--full): the rank's batched local steps alone (no in-rank fold, no
    # collective), replayed over the same plan steps after the run
    steps_ms = None
    rr = out["round"]
    if args.full and hasattr(rr, "time_local_steps") and args.backend == "fused":
        steps_ms = rr.time_local_steps(args.warmup, min(args.steps, 500))
    # (every rank joins the reduction, also one that hosts a single client)
    steps_ms = _max_over_ranks(-1.0 if steps_ms is None else steps_ms, world)
    steps_ms = None if steps_ms < 0 else steps_ms
    rr.close()
    # ---- quality (--full): a separate untimed federation of --npmi-steps rounds ----
    quality = _quality(args, corpora, ids, sc, n_clients, rank, device, kw)
    if rank == 0:
        ms = wall / max(out["timed_rounds"], 1) * 1e3
        rec = _record(args, docs / wall, ms, len(out["clients"][0].tm.train_data.idx2token),
                      quality.get("npmi"), final_loss, clients=n_clients, ranks=world,
                      physical=physical)
        rec.update({k: v for k, v in quality.items() if k != "npmi"})
        rec["device_ms_per_step"] = (None if dev_s is None else
                                     round(dev_s / max(out["timed_rounds"], 1) * 1e3, 5))
        per_rank = sorted({len(b) for b in assign_clients(n_clients, world)})
        rec["config"]["aggregation"] += (
            f" ({'/'.join(map(str, per_rank))} client(s) per rank"
            + (", batched steps + in-rank fold" if per_rank[-1] > 1 else "")
            + f", {out['allreduce'] or 'no'} all-reduce across ranks)")
        rec["path"] = "run_distributed"
        rec["engine_ran"] = out["clients"][0].tm.engine_info
        # the in-rank FedAvg of a multi-client rank: inside the update kernels' epilogues
        # (csrc gfk_bwd_fold_k / gfk_win_fold_k) or the fold kernel after the batched steps
        rec["fedavg_plan"] = getattr(out["round"], "fold_plan", None)
        split = {"round_ms": round(ms, 5)}
        if rec["device_ms_per_step"] is not None:
            split["device_ms"] = rec["device_ms_per_step"]
            split["host_ms"] = round(max(ms - rec["device_ms_per_step"], 0.0), 5)
            if steps_ms is not None:
                # the local steps with per-client updates alone, and what the round's FedAvg
                # (the in-rank fold -- a kernel, or inside the update epilogues -- and the
                # collective) adds to them on the device (negative: the in-epilogue FedAvg's
                # kernels beat the per-client update kernels they replace)
                split["local_steps_device_ms"] = round(steps_ms, 5)
                split["fedavg_device_ms"] = round(rec["device_ms_per_step"] - steps_ms, 5)
        rec["round_split_ms"] = split
        rec["digests"] = out.get("digests")
        if fallback:
            rec["allreduce_fallback"] = fallback
        if out.get("attach"):
            rec["fedavg_attach"] = out["attach"]
        if rehearse:
            rec["note"] = (f"GFEDNTM_REHEARSE_1GPU: {world} ranks share {physical} GPU -- "
                           "protocol rehearsal, timings meaningless")
        print(json.dumps(rec), flush=True)
    dist.barrier(group=_ctrl_group())
    dist.destroy_process_group()


def _quality(args, corpora, ids, sc, n_clients, rank, device, kw) -> dict:
    """NPMI (top-10 words of client 1's topics over every client's documents) and client
    1's TSS / DSS against the generator's ground truth, from a separate untimed federation
    of --npmi-steps rounds, so the numbers do not depend on --steps."""
    if not args.full or args.no_npmi or args.npmi_steps <= 0:
        return {}
    from gfedntm_amd.federation.hierarchical import run_distributed_multi
    out = run_distributed_multi(corpora, ids, _params(args), _model_type(args),
                                max_iters=args.npmi_steps, **kw)
    q = {}
    if rank == 0:
        c = out["clients"][0]
        q["npmi"] = _npmi(c.tm, sc, _union_terms(sc, n_clients), n_clients, device)
        if args.family == "avitm":
            c.ground_truth = (np.asarray(sc.doc_topics[c.id - 1]), np.asarray(sc.topic_vectors))
            betas, thetas, _ = c.results()
            ev = c.evaluate_synthetic(betas, thetas)
            q["tss_client1"] = round(ev["tss"], 4)
            q["dss_client1"] = round(ev["dss"], 4)
    return q


def run_federated(args):
    from gfedntm_amd.federation.runner import CommError, run_distributed
    rank, world, device, rehearse = _init(args)
    _ctrl_group()
    if total_clients(args, world) != world:
        return run_multi(args, rank, world, device, rehearse)
    physical = _physical_gpus(device, world)
    sc = _corpus(args, world)
    corpus = _client_corpus(args, sc, rank)
    params = _params(args)
    n_rounds = args.warmup + args.steps
    kw = dict(params=params, model_type=_model_type(args), backend=args.backend,
              seed=args.seed, graph=not args.no_graph, allreduce=args.allreduce,
              rehearse_1gpu=rehearse)
    # ---- timed: the production round loop ----
    fallback = None
    try:
        out = run_distributed(corpus, max_iters=n_rounds, timing_warmup=args.warmup,
                              keep_round=True, **kw)
    except CommError as e:
        # every rank raised the same agreed error: an xGMI wait timed out.  With the data
        # plane left to auto-selection, measure the same federation over RCCL instead (and
        # say so in the record) rather than reporting nothing
        if args.allreduce not in (None, "auto"):
            raise
        fallback = f"xGMI all-reduce failed ({e}); re-run over RCCL"
        if rank == 0:
            print(f"[bench] {fallback}", file=sys.stderr, flush=True)
        kw["allreduce"] = "rccl"
        # a failure injection (tests) belongs to the failed attempt, not the re-measure
        os.environ.pop("GFEDNTM_INJECT_STALL", None)
        os.environ.pop("GFEDNTM_INJECT_CORRUPT", None)
        out = run_distributed(corpus, max_iters=n_rounds, timing_warmup=args.warmup,
                              keep_round=True, **kw)
    client = out["client"]
    eng = client.tm.engine
    wall = _max_over_ranks(out["wall_s"], world)
    dev_s = out.get("device_s")
    dev_s = None if dev_s is None else _max_over_ranks(dev_s, world)
    timed_rounds = out["timed_rounds"]
    t = torch.tensor([float(out["docs"])], dtype=torch.float64)
    dist.all_reduce(t, group=_ctrl_group())
    docs = float(t.item())                       # all clients' training documents
    ms_runner = wall / max(timed_rounds, 1) * 1e3
    if args.path != "engine":
        _dump_outputs(args, [client], n_rounds - 1, world)
    # ---- the same engine's bare replay loop (collective still attached): the headline of
    # --path engine, a side measurement (--full) of --path runner ----
    engine_ms = engine_dev_ms = compute_ms = None
    if args.backend == "fused" and (args.full or args.path == "engine"):
        dt, ddev = _engine_loop(eng, args.warmup, n_rounds, world)
        engine_ms, engine_dev_ms = dt / args.steps * 1e3, ddev / args.steps * 1e3
        err = eng.fedavg_error()
        if args.path == "engine":
            _dump_outputs(args, [client], n_rounds - 1, world)
        if world > 1 and args.full:
            # round split: the same steps again with the collective detached
            saved = eng.detach_fedavg(close=False)
            _, ddev2 = _engine_loop(eng, args.warmup, n_rounds, world)
            compute_ms = ddev2 / args.steps * 1e3
            eng.restore_fedavg(saved)
        if err:
            raise RuntimeError(f"xGMI all-reduce reported error {err}")
    used = out["allreduce"]
    final_loss = float(np.mean(eng.loss_hist[max(0, n_rounds - 20): n_rounds].cpu().numpy()))
    if args.backend == "fused":
        eng.detach_fedavg()
    # ---- quality (--full): a separate untimed federation of a fixed number of rounds ----
    quality = _quality(args, [corpus], [rank + 1], sc, world, rank, device,
                       {k: v for k, v in kw.items() if k not in ("params", "model_type")})
    npmi = quality.get("npmi")
    if rank == 0:
        value = docs / wall
        terms_n = len(client.tm.train_data.idx2token) if hasattr(client.tm.train_data, "idx2token") \
            else client.tm.input_size
        out_digests = out.get("digests")
        record = _record(args, value, ms_runner, terms_n, npmi, final_loss, clients=world,
                         ranks=world, physical=physical)
        record.update({k: v for k, v in quality.items() if k != "npmi"})
        record["path"] = args.path
        record["engine_ran"] = client.tm.engine_info
        record["digests"] = out_digests
        if fallback:
            record["allreduce_fallback"] = fallback
        record["device_ms_per_step"] = None if dev_s is None else round(dev_s / max(timed_rounds, 1) * 1e3, 5)
        record["engine_only_ms_per_step"] = None if engine_ms is None else round(engine_ms, 5)
        record["engine_only_device_ms_per_step"] = (None if engine_dev_ms is None
                                                    else round(engine_dev_ms, 5))
        record["runner_overhead_pct"] = (None if engine_dev_ms is None or dev_s is None else
                                         round(100.0 * (dev_s / max(timed_rounds, 1) * 1e3
                                                        / engine_dev_ms - 1.0), 2))
        if args.path == "engine" and engine_ms is not None:
            # headline from the bare replay loop instead
            record["ms_per_step"] = round(engine_ms, 5)
            record["value"] = round(world * args.batch / (engine_ms * 1e-3), 1)
            if record["vs_baseline"] is not None:
                record["vs_baseline"] = round(record["value"] / BASELINE_FED_DOCS_PER_S, 2)
        record["config"]["aggregation"] += f" ({used or 'none: one client'} all-reduce)"
        if out.get("attach"):
            record["fedavg_attach"] = out["attach"]
        _ctx_note(record, args, eng)
        split = {"round_ms": round(record["ms_per_step"], 5)}
        if compute_ms is not None:
            split["compute_device_ms"] = round(compute_ms, 5)
            split["allreduce_exposed_device_ms"] = round(max(engine_dev_ms - compute_ms, 0.0), 5)
        if record["device_ms_per_step"] is not None:
            split["host_ms"] = round(max(ms_runner - record["device_ms_per_step"], 0.0), 5)
        record["round_split_ms"] = split
        if rehearse:
            record["note"] = (f"GFEDNTM_REHEARSE_1GPU: {world} ranks share {physical} GPU -- "
                              "protocol rehearsal, timings meaningless")
        print(json.dumps(record), flush=True)
    dist.barrier(group=_ctrl_group())
    dist.destroy_process_group()


def run_simulated(args):
    """M simulated clients on one GPU (LocalFederation round graph)."""
    from gfedntm_amd.federation.runner import LocalFederation
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    M = args.sim_clients
    sc = _corpus(args, M)
    corpora = [_client_corpus(args, sc, i) for i in range(M)]
    n_rounds = args.warmup + args.steps
    fed = LocalFederation(corpora, _params(args), _model_type(args), n_rounds, device=device,
                          backend=args.backend, seed=args.seed, graph=not args.no_graph,
                          round_streams=not args.serial_clients,
                          round_batched=not args.unbatched)
    out = fed.run(timing_warmup=args.warmup)
    ms = out["wall_s"] / max(out["timed_rounds"], 1) * 1e3
    value = out["docs"] / out["wall_s"]
    _dump_outputs(args, fed.clients, n_rounds - 1, M)
    npmi = None
    if args.full and not args.no_npmi and args.npmi_steps > 0:
        fed2 = LocalFederation(corpora, _params(args), _model_type(args), args.npmi_steps,
                               device=device, backend=args.backend, seed=args.seed,
                               graph=not args.no_graph, round_streams=not args.serial_clients)
        fed2.run()
        npmi = _npmi(fed2.clients[0].tm, sc, fed.terms, M, device)
    eng = fed.clients[0].tm.engine
    final_loss = float(np.mean(eng.loss_hist[max(0, n_rounds - 20): n_rounds].cpu().numpy()))
    rec = _record(args, value, ms, len(fed.terms), npmi, final_loss, clients=M, ranks=1,
                  physical=1)
    if out.get("device_s") is not None:
        rec["device_ms_per_step"] = round(out["device_s"] / max(out["timed_rounds"], 1) * 1e3, 5)
    mode = ("batched kernels (grid z = client)" if fed._batched is not None else
            "client branches" if not args.serial_clients else "serial clients")
    rec["config"]["aggregation"] += (f" (in-process FedAvg kernel in one round graph, {mode})"
                                     if fed.round_graph else " (eager)")
    rec["path"] = "LocalFederation"
    rec["engine_ran"] = fed.clients[0].tm.engine_info
    _ctx_note(rec, args, eng)
    print(json.dumps(rec), flush=True)


def _ctx_note(rec, args, eng):
    """CTM lines say whether the contextual path ran on the fused kernels or on the
    host-GEMM fallback (and why)."""
    if args.family == "avitm" or args.backend != "fused":
        return
    why = getattr(eng, "ctx_fallback_reason", None)
    rec["ctx_path"] = "fused kernels" if why is None else f"host-GEMM fallback: {why}"
    if getattr(eng, "ctx_gemm_dtype", None):
        rec["ctx_gemm_dtype"] = eng.ctx_gemm_dtype


def _is_headline(args) -> bool:
    return all(getattr(args, k) == v for k, v in HEADLINE.items())


def _metric(args, V, clients: int, ranks: int, physical: int) -> str:
    """BASELINE.json's metric string for the headline config -- exactly 8 federated clients,
    each rank on its own GPU; otherwise a label derived from what actually ran."""
    if _is_headline(args) and clients == 8 and physical == ranks:
        return METRIC
    fam = {"avitm": "ProdLDA" if args.model == "prodLDA" else "NeuralLDA",
           "ctm": "CombinedTM", "zeroshot": "ZeroShotTM"}[args.family]
    ctx = f" C={args.contextual_size}" if args.family != "avitm" else ""
    where = (f"{clients} clients" + (f" on {ranks} ranks" if ranks != clients else "")
             + f" on {physical} GPU" + ("s" if physical != 1 else ""))
    return (f"docs/sec (whole node), {fam} K={args.topics} V={V} H=({args.hidden}){ctx} "
            f"{args.dtype}, {where}, synthetic BoW")


def _kernels_hash(args):
    if args.backend != "fused":
        return None
    from gfedntm_amd.ops import native
    return native.kernels_hash()


def _record(args, value, ms, V, npmi, final_loss, clients: int, ranks: int, physical: int):
    hidden = tuple(int(h) for h in args.hidden.split(","))
    fam = {"avitm": "", "ctm": "CombinedTM-", "zeroshot": "ZeroShotTM-"}[args.family]
    ctx = f" C={args.contextual_size}" if args.family != "avitm" else ""
    metric = _metric(args, V, clients, ranks, physical)
    headline = metric == METRIC
    return {
        "metric": metric,
        "value": round(value, 1),
        "unit": "docs/s",
        "n_gpus": physical,
        "ranks": ranks,
        "physical_gpus": physical,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms, 5),
        "higher_is_better": True,
        # --clients (default): the 8-client federation whatever N -- total work fixed;
        # --clients-per-gpu: M clients on every GPU -- per-GPU work fixed
        "scaling": "weak" if args.clients_per_gpu else "strong",
        # only the headline config is comparable with the reference's 8-client number
        "vs_baseline": round(value / BASELINE_FED_DOCS_PER_S, 2) if headline else None,
        "dtype": args.dtype,
        "data": (f"synthetic (reference LDA generator: V={args.vocab}, K={args.topics}, "
                 f"{args.docs} docs/client, {args.nwords.replace(',', '-')} tokens, "
                 "5 frozen topics), random init"),
        "config": {"model": f"{fam}{args.model}{ctx} K={args.topics} H={hidden} V={V}",
                   "global_batch": args.batch * clients, "seq_len": None,
                   "per_client_batch": args.batch, "clients": clients,
                   "parallelism": (f"fedavg-dp{clients}" if clients == ranks else
                                   f"fedavg {clients} clients / {ranks} ranks"),
                   "backend": args.backend + ("" if args.no_graph else "+hipgraph"),
                   "solver": args.solver,
                   "aggregation": "per-minibatch sample-weighted FedAvg of the shared state"},
        "clients_note": (f"{clients} federated client(s) on {ranks} rank(s) / {physical} "
                         f"physical GPU(s): every round all {clients} clients do one local "
                         "minibatch step and the sample-weighted FedAvg of their shared state "
                         "replaces every client's copy"),
        **({"precision": "bf16 operands of the ProdLDA decoder GEMMs (theta.beta, theta^T.dlogit, "
                         "dlogit.beta^T) and, for CombinedTM, of the contextual forward GEMMs "
                         "(x_ctx.Wa^T, A.Wc^T; see ctx_gemm_dtype) on v_mfma_f32_16x16x32_bf16, "
                         "fp32 accumulation; fp32 parameters, Adam state and every other op"}
           if args.dtype == "bf16" else {}),
        # the source hash embedded in the kernel library that ran (gfedntm_amd/ops/srchash.py)
        "kernels_src_hash": _kernels_hash(args),
        "npmi": None if npmi is None else round(npmi, 4),
        "npmi_rounds": None if npmi is None else args.npmi_steps,
        "final_loss": final_loss,
        "baseline": {"fed_grpc_8clients_docs_per_s": BASELINE_FED_DOCS_PER_S,
                     "cpu_centralized_docs_per_s": BASELINE_CPU_CENTRALIZED_DOCS_PER_S},
    }

def run(args):
    if args.sim_clients:
        return run_simulated(args)
    return run_federated(args)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    if args.clients_per_gpu is None and args.clients < 1:
        raise SystemExit("--clients must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.sim_clients:
        # self-launch: one rank per GPU, spawned before this process touches the GPU
        import torch.multiprocessing as mp
        port = _free_port()
        mp.start_processes(_spawned, args=(args.gpus, port, argv), nprocs=args.gpus,
                           start_method="spawn")
        return
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws != args.gpus and not args.sim_clients:
        print(f"bench.py: WORLD_SIZE={ws} overrides --gpus {args.gpus}", file=sys.stderr)
    run(args)


if __name__ == "__main__":
    main()
