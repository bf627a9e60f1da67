"""float64 numpy oracle of held-out scoring, written out from a model's ``state_dict``
(shared by tests/test_score.py and tests/test_score_gpu.py; not a test module).

Eval mode throughout: batch-norm with running statistics, no dropout; the encoder is the
oracle of tests/infer_oracle.py (every activation, any depth, CTM and label inputs).
"""
import numpy as np

from tests.infer_oracle import np_state, oracle_moments  # noqa: F401  (re-exported)


def _softmax(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def _logsumexp(z):
    m = z.max(-1, keepdims=True)
    return m + np.log(np.exp(z - m).sum(-1, keepdims=True))


def oracle_score(tm, X, eps=None, ctx=None, labels=None):
    """Per-document ELBO terms in float64.  ``eps``: normals [S, D, K], or None for the
    plug-in theta = softmax(mu).  Returns a dict: ``kl``, ``rl`` [D] (RL: the mean over the
    draws), ``ce`` [D] (label-head models), ``zn_absmax`` (ProdLDA: the largest |BN'ed
    logit|) and ``p_nz_min`` / ``p_nz_max`` (the smallest / largest word probability at a
    scored non-zero)."""
    sd = np_state(tm)
    K = tm.n_components
    x = np.asarray(X.toarray(), dtype=np.float64)
    mu, ls = oracle_moments(tm, X, ctx, labels)
    pm = tm.model.prior_mean.detach().double().cpu().numpy()
    pv = tm.model.prior_variance.detach().double().cpu().numpy()
    kl = 0.5 * ((np.exp(ls) / pv).sum(1) + ((pm - mu) ** 2 / pv).sum(1) - K
                + np.log(pv).sum() - ls.sum(1))
    beta = sd["beta"]
    rm, rv = sd["beta_batchnorm.running_mean"], sd["beta_batchnorm.running_var"]
    bn_eps = tm.model.beta_batchnorm.eps
    draws = [mu] if eps is None else [mu + np.asarray(e, dtype=np.float64) * np.exp(0.5 * ls)
                                      for e in eps]
    out = {"kl": kl, "rl": np.zeros(len(kl)), "zn_absmax": 0.0, "p_nz_min": np.inf,
           "p_nz_max": 0.0}
    ce = np.zeros(len(kl)) if labels is not None and getattr(tm, "label_size", 0) else None
    for z in draws:
        theta = _softmax(z)
        if tm.model.is_prodlda:
            zn = (theta @ beta - rm) / np.sqrt(rv + bn_eps)
            p = np.exp(zn - _logsumexp(zn))
            out["zn_absmax"] = max(out["zn_absmax"], float(np.abs(zn).max()))
        else:
            p = theta @ _softmax((beta - rm) / np.sqrt(rv + bn_eps))
        out["rl"] += -(x * np.log(p + 1e-10)).sum(1)
        if (x > 0).any():
            out["p_nz_min"] = min(out["p_nz_min"], float(p[x > 0].min()))
            out["p_nz_max"] = max(out["p_nz_max"], float(p[x > 0].max()))
        if ce is not None:
            logits = theta @ sd["label_classification.weight"].T + sd["label_classification.bias"]
            target = np.argmax(np.asarray(labels), 1)
            ce += (_logsumexp(logits)[:, 0] - logits[np.arange(len(target)), target])
    out["rl"] /= len(draws)
    if ce is not None:
        out["ce"] = ce / len(draws)
    return out


def oracle_loss(kl, rl, kl_weight=1.0, ce=None, batch_size=64):
    """mean over documents of kl_weight KL + RL, plus the label CE (the mean of every
    ``batch_size`` documents, one term per minibatch) where there is one."""
    tot = float(np.sum(kl_weight * kl + rl))
    if ce is not None:
        tot += sum(float(ce[a:a + batch_size].mean()) for a in range(0, len(ce), batch_size))
    return tot / len(kl)


def oracle_perplexity(kl, rl, X):
    return float(np.exp(np.sum(kl + rl) / X.sum()))
