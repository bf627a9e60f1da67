"""Oracles for the Gibbs LDA sampler (ops/lda.py, csrc/gibbs.hip): a float64 teacher-forced
replay of a sweep, the count identities, a seeded LDA corpus generator with its quality
score, and the textbook serial collapsed sampler.  Nothing here imports the code under test:
the Philox draws are reproduced by an implementation of its own."""
import functools

import numpy as np
import scipy.sparse as sp

RNG_GIBBS = 7
R = 2.0 ** -24                       # fp32 unit roundoff


def delta(K):
    """The sweep oracle's relative bound (docs/PARITY.md §4.3): (K + 16) 2^-24."""
    return (K + 16) * R


# --------------------------------------------------------------------------- Philox
def _philox(seed, c):
    """Philox4x32-10 on python-int-safe uint64 arrays; c = four arrays of 32-bit words."""
    m = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) for v in c]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m, p1 & m,
             ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m, p0 & m]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c


def draws(seed, sweep, doc, pos):
    """u (float64, exact multiples of 2^-24) of tokens ``pos`` of global documents ``doc``."""
    doc, pos = np.asarray(doc, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    n = len(doc)
    r = _philox(int(seed) % (1 << 64), [doc, np.full(n, sweep), RNG_GIBBS | ((pos >> 2) << 8),
                                        np.full(n, 0x5EED)])
    x = np.stack(r)[pos & 3, np.arange(n)]
    return (x >> np.uint64(8)).astype(np.float64) / 16777216.0


# --------------------------------------------------------------------------- tokens
class Tokens:
    """The sampler's token order: document by document, the CSR row in storage order, a
    non-zero (w, x) as x consecutive tokens."""

    def __init__(self, csr):
        csr = sp.csr_matrix(csr)
        x = csr.data.astype(np.int64)
        assert np.all(x == csr.data) and np.all(x >= 0)
        self.D, self.V = csr.shape
        rows = np.repeat(np.arange(self.D), np.diff(csr.indptr))
        self.doc = np.repeat(rows, x)
        self.word = np.repeat(csr.indices.astype(np.int64), x)
        lens = np.bincount(self.doc, minlength=self.D)
        self.N = int(lens.sum())
        self.pos = np.arange(self.N) - np.repeat(np.cumsum(lens) - lens, lens)
        order = np.argsort(self.pos, kind="stable")
        self.by_pos = np.split(order, np.cumsum(np.bincount(self.pos))[:-1]) if self.N else []


def counts(tok, z, K):
    """(nwk, nk, ndk) int64 of assignments z."""
    z = np.asarray(z, dtype=np.int64)
    nwk = np.bincount(tok.word * K + z, minlength=tok.V * K).reshape(tok.V, K)
    ndk = np.bincount(tok.doc * K + z, minlength=tok.D * K).reshape(tok.D, K)
    return nwk, nwk.sum(0), ndk


def initial_z(tok, K, seed, doc0=0):
    """Sweep 0: min(K - 1, floor(u K)) with the product rounded to fp32."""
    u = draws(seed, 0, doc0 + tok.doc, tok.pos).astype(np.float32)
    return np.minimum(K - 1, np.floor(u * np.float32(K)).astype(np.int64))


def sweep_rejects(tok, z0, z1, nwk0, nk0, alpha, beta, seed, sweep, frozen=False, doc0=0):
    """Teacher-forced float64 replay of one sweep z0 -> z1 against the start-of-sweep counts:
    at every token the state the sampler's own choices imply gives C_k = sum_{j <= k} p_j and
    T = C_{K-1}; the sampler's k* is accepted iff
        C_{k*-1} (1 - delta) <= u T (1 + delta)  and  u T (1 - delta) < C_{k*} (1 + delta)
    (the second waived at k* = K - 1).  Returns the number of rejected tokens: every token is
    checked, and a rejected one does not disturb the next (the replay follows z1)."""
    z0, z1 = np.asarray(z0, dtype=np.int64), np.asarray(z1, dtype=np.int64)
    K = len(alpha)
    dl = delta(K)
    a = np.asarray(alpha, dtype=np.float32).astype(np.float64)
    b = float(np.float32(beta))
    vb = tok.V * b
    nwk0, nk0 = np.asarray(nwk0, dtype=np.int64), np.asarray(nk0, dtype=np.int64)
    _, _, nd = counts(tok, z0, K)
    u_all = draws(seed, sweep, doc0 + tok.doc, tok.pos)
    bad = 0
    for idx in tok.by_pos:
        d, w, o, k = tok.doc[idx], tok.word[idx], z0[idx], z1[idx]
        r = np.arange(len(idx))
        nd[d, o] -= 1
        ex = np.zeros((len(idx), K))
        if not frozen:
            ex[r, o] = 1.0
        p = (nd[d] + a) * (nwk0[w] - ex + b) / (nk0[None, :] - ex + vb)
        C = np.cumsum(p, axis=1)
        ut = u_all[idx] * C[:, -1]
        lo = np.where(k > 0, C[r, np.maximum(k - 1, 0)], 0.0)
        ok = (lo * (1 - dl) <= ut * (1 + dl)) & ((k == K - 1) | (ut * (1 - dl) < C[r, k] * (1 + dl)))
        ok &= (k >= 0) & (k < K)
        bad += int((~ok).sum())
        nd[d, k] += 1
    return bad


# --------------------------------------------------------------------------- quality
def lda_corpus(D, V, K, mean_len, seed, alpha=0.1, eta=0.02):
    """A corpus drawn from LDA: (csr float32, phi [K, V])."""
    rng = np.random.default_rng(seed)
    phi = rng.dirichlet(np.full(V, eta), size=K)
    x = np.zeros((D, V), dtype=np.float32)
    for d in range(D):
        theta = rng.dirichlet(np.full(K, alpha))
        n = max(1, rng.poisson(mean_len))
        zs = rng.choice(K, size=n, p=theta)
        for k in np.unique(zs):
            x[d] += rng.multinomial(int((zs == k).sum()), phi[k])
    return sp.csr_matrix(x), phi


def score(phi_true, phi):
    """Mean over the true topics of the best Bhattacharyya coefficient sum_w sqrt(phi_true phi)."""
    return float((np.sqrt(phi_true) @ np.sqrt(phi).T).max(1).mean())


def serial_gibbs(csr, K, alpha, beta, sweeps, seed):
    """The textbook serial collapsed sampler (every count live): phi [K, V]."""
    tok = Tokens(csr)
    rng = np.random.default_rng(seed)
    z = rng.integers(0, K, size=tok.N)
    nwk, nk, ndk = counts(tok, z, K)
    nwk, nk, ndk = nwk.astype(np.float64), nk.astype(np.float64), ndk.astype(np.float64)
    vb = tok.V * beta
    us = rng.random((sweeps, tok.N))
    for s in range(sweeps):
        for i in range(tok.N):
            d, w, o = tok.doc[i], tok.word[i], z[i]
            nwk[w, o] -= 1; nk[o] -= 1; ndk[d, o] -= 1
            c = np.cumsum((ndk[d] + alpha) * (nwk[w] + beta) / (nk + vb))
            k = min(K - 1, int(np.searchsorted(c, us[s, i] * c[-1], side="right")))
            z[i] = k
            nwk[w, k] += 1; nk[k] += 1; ndk[d, k] += 1
    return ((nwk + beta) / (nk + vb)).T


SMALL = dict(D=60, V=20, K=3, mean_len=17)
MEDIUM = dict(D=300, V=400, K=8, mean_len=60)
QUALITY = dict(alpha=0.1, beta=0.02, sweeps=100)      # alpha per topic
# the serial sampler's two-seed minimum on MEDIUM (corpus seed 0; sampler seeds 0 and 1 gave
# 0.99219 and 0.99198), run once: docs/PARITY.md §4.3
MEDIUM_SERIAL_MIN = 0.99198


@functools.lru_cache(maxsize=None)
def small_case():
    """(csr, phi_true, the serial sampler's score) of the small quality case."""
    csr, phi = lda_corpus(seed=0, **SMALL)
    ref = serial_gibbs(csr, SMALL["K"], QUALITY["alpha"], QUALITY["beta"], QUALITY["sweeps"], 0)
    return csr, phi, score(phi, ref)
