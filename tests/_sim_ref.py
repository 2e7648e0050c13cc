"""Shared by the similarity-prediction tests: a numpy/scipy statement of the reference's ground truth (the adjacency it builds and
the Leicht–Holme–Newman series with its finish steps), written from the algorithm, for small graphs."""
import numpy as np
import scipy.sparse as sp


def adjacency(src, dst, w, n):
    """The reference's matrix of snapshot rows: a lil matrix where every row sets A[u, v] = A[v, u] = w in file order (assigning 0
    removes the entry), self loops skipped, then CSR."""
    A = sp.lil_matrix((n, n))
    for u, v, x in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(w, np.float64).tolist()):
        if u == v:
            continue
        A[u, v] = x
        A[v, u] = x
    return A.tocoo().tocsr()


def similarity(A, lam, alpha=0.5, iter_num=100):
    """The n x n similarity as scipy COO: iter_num steps of S = c·(A·S) + I from S = 0 with c = alpha / lam (scipy's CSR x dense
    product), then (S + Sᵀ)/2, minus I, min-max over all entries, entries below 1e-6 set to 0."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    c = alpha / lam
    eye = np.eye(n)
    S = np.zeros((n, n))
    for _ in range(iter_num):
        S = c * A.dot(S) + eye
    S = (S + S.T) / 2
    S = S - eye
    S = (S - S.min()) / (S.max() - S.min())
    S[S < 1e-6] = 0
    return sp.coo_matrix(S)
