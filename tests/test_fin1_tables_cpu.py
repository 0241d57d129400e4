"""The algebra of BN1's moments without the lag-Gram matrix, in float64 numpy: the identity a table-based
fin1 rests on (the kernels still build the Gram, eegnet_finalize.hip fin1_body).

Pass A publishes, per batch, the lag sums of the zero-padded rows X (left pad P = (K1 - 1) // 2, right
pad R = K1 - 1 - P): G0[d] = sum X[s] X[s + d] over s < T, S0 = sum X[s], and the edge terms -- head
pairs H[a][b] = sum_c x[a] x[b] (a <= b < R), tail pairs Tl[u][v] = sum_c x[T - P + u] x[T - P + v]
(u <= v < P), head sums hs, tail sums ts.  The Gram of the K1 shifted windows and the window sums are

    G[k][k + d] = G0[d] + sum_{j < k} Ed[d][j],   Ed[d][j] = X[T + j] X[T + j + d] - X[j] X[j + d]
    S1[k]       = S0 + sum_{j < k} es[j],         es[j]    = X[T + j] - X[j]

so with m_0 = 1, m_d = 2 (d >= 1) and the parameter-only tables

    A[d]    = sum_{k = 0}^{K1 - 1 - d} w_k w_{k + d}
    U[d][j] = sum_{k = j + 1}^{K1 - 1 - d} w_k w_{k + d}
    V[j]    = sum_{k > j} w_k

    w^T G w  = sum_d m_d (G0[d] A[d] + sum_j Ed[d][j] U[d][j])
    w^T S1   = S0 sum_k w_k + sum_j es[j] V[j]

Checked against the explicitly built Gram / window sums of the padded rows to 1e-12 relative, at K1 = 32
and 64, T = 64 (with K1 = 64 every sample is an edge sample of some window), 256 and 257, C = 1 and 22."""

from __future__ import annotations

import numpy as np
import pytest


def pass_a_sums(x, K1):
    """The parameter-free sums pass A publishes for trials x [B, C, T] (float64)."""
    B, C, T = x.shape
    P = (K1 - 1) // 2
    R = K1 - 1 - P
    X = np.zeros((B, C, T + K1 - 1))
    X[:, :, P:P + T] = x
    G0 = np.array([np.sum(X[:, :, :T] * X[:, :, d:d + T]) for d in range(K1)])
    S0 = float(np.sum(X[:, :, :T]))
    H = {(a, b): float(np.sum(x[:, :, a] * x[:, :, b])) for a in range(R) for b in range(a, R)}
    Tl = {(u, v): float(np.sum(x[:, :, T - P + u] * x[:, :, T - P + v])) for u in range(P) for v in range(u, P)}
    hs = np.array([np.sum(x[:, :, a]) for a in range(R)])
    ts = np.array([np.sum(x[:, :, T - P + u]) for u in range(P)])
    return X, G0, S0, H, Tl, hs, ts


def edge_terms(K1, H, Tl, hs, ts):
    """Ed[d][j] (j <= K1 - 2 - d) and es[j] (j <= K1 - 2) from the published edge sums, with fin1's index
    rules: X[T + j] is sample T - P + j (j < P, else pad), X[j] is sample j - P (j >= P, else pad)."""
    P = (K1 - 1) // 2
    Ed = np.zeros((K1, K1))
    for d in range(K1):
        for j in range(K1 - 1 - d):
            t = Tl[(j, j + d)] if j + d < P else 0.0
            h = H[(j - P, j - P + d)] if j >= P else 0.0
            Ed[d, j] = t - h
    es = np.array([(ts[j] if j < P else 0.0) - (hs[j - P] if j >= P else 0.0) for j in range(K1 - 1)])
    return Ed, es


def tap_tables(w):
    """A[d], U[d][j], V[j] of one filter's taps w [K1] (parameter-only)."""
    K1 = len(w)
    A = np.zeros(K1)
    U = np.zeros((K1, K1))
    for d in range(K1):
        pr = w[:K1 - d] * w[d:]                       # pr[k] = w_k w_{k+d}, k <= K1 - 1 - d
        A[d] = pr.sum()
        for j in range(K1 - 1 - d):
            U[d, j] = pr[j + 1:].sum()
    V = np.array([w[j + 1:].sum() for j in range(K1 - 1)])
    return A, U, V


@pytest.mark.parametrize("K1", [32, 64])
@pytest.mark.parametrize("T", [64, 256, 257])
@pytest.mark.parametrize("C", [1, 22])
def test_table_moments_equal_explicit_gram(K1, T, C):
    rng = np.random.default_rng(1000 * K1 + 10 * T + C)
    B, F1 = 3, 4
    x = rng.standard_normal((B, C, T))
    w1 = rng.standard_normal((F1, K1)) / np.sqrt(K1)
    X, G0, S0, H, Tl, hs, ts = pass_a_sums(x, K1)
    # explicit Gram and window sums of the padded rows
    win = np.stack([X[:, :, k:k + T] for k in range(K1)])            # [K1, B, C, T]
    G = np.einsum("kbct,lbct->kl", win, win)
    S1 = win.sum(axis=(1, 2, 3))
    Ed, es = edge_terms(K1, H, Tl, hs, ts)
    # the identities themselves
    for d in range(K1):
        diag = np.array([G[k, k + d] for k in range(K1 - d)])
        np.testing.assert_allclose(diag, G0[d] + np.concatenate([[0.0], np.cumsum(Ed[d, :K1 - 1 - d])]),
                                   rtol=1e-12, atol=1e-12 * abs(G0[0]))
    np.testing.assert_allclose(S1, S0 + np.concatenate([[0.0], np.cumsum(es)]), rtol=1e-12,
                               atol=1e-12 * np.abs(X).sum())
    md = np.where(np.arange(K1) == 0, 1.0, 2.0)
    for f in range(F1):
        w = w1[f]
        A, U, V = tap_tables(w)
        q = float(np.sum(md * (G0 * A + np.sum(Ed * U, axis=1))))
        m = S0 * w.sum() + float(np.sum(es * V))
        q_ref, m_ref = float(w @ G @ w), float(w @ S1)
        assert abs(q - q_ref) <= 1e-12 * abs(q_ref), (f, q, q_ref)
        assert abs(m - m_ref) <= 1e-12 * abs(m_ref), (f, m, m_ref)
