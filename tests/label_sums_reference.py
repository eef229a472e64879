"""The label-sum contract of include/voxproj_cluster.h in NumPy (shared by test_label_sums_cpu.py and the GPU tests), the
float64 spherical k-means the product's loop is compared with, and the planted scenes both suites cluster.

    a[r,c]      = fl32( fl32(x[r,c]) * s_r )
    part(k, p)  = the rows of label k in ascending row index, positions [p R, min((p + 1) R, n_k))
    partial     = (((+0 + a[r0,c]) + a[r1,c]) + a[r2,c]) + ...          float32, in that order
    sums[k,c]   = fl32( +0 + the float64 sum of the label's partials in ascending p )
    R           = part_rows, or max(256, ceil(n_rows / 32768)) when part_rows = 0
"""
import numpy as np


def default_part_rows(n_rows):
    return max(256, -(-int(n_rows) // 32768))


def label_sums(rows, labels, K, row_scale=None, part_rows=0):
    """(sums f32 [K,C], counts i32 [K], status i32 [2]) of the contract.  rows float16 or float32 [N,C]."""
    x = np.asarray(rows)
    assert x.dtype in (np.float16, np.float32) and x.ndim == 2
    x = x.astype(np.float32)                                         # binary16 -> float32 is exact
    labels = np.asarray(labels, dtype=np.int64)
    N, C = x.shape
    R = int(part_rows) if part_rows else default_part_rows(N)
    if row_scale is not None:
        x = x * np.asarray(row_scale, dtype=np.float32)[:, None]     # float32 * float32 -> float32: one rounding
    sums = np.zeros((K, C), np.float32)
    counts = np.zeros(K, np.int32)
    status = np.array([(labels < 0).sum(), (labels >= K).sum()], np.int32)
    order = np.argsort(labels, kind="stable")
    lab = labels[order]
    for k in np.unique(lab[(lab >= 0) & (lab < K)]):
        idx = order[np.searchsorted(lab, k, "left"):np.searchsorted(lab, k, "right")]          # ascending row index
        counts[k] = len(idx)
        total = np.zeros(C, np.float64)
        for p in range(0, len(idx), R):
            part = np.zeros(C, np.float32)
            for r in idx[p:p + R]:
                part = part + x[r]                                   # float32 + float32, row by row
            total = total + part.astype(np.float64)
        sums[k] = total.astype(np.float32)
    return sums, counts, status


def sums64(rows, labels, K, row_scale=None):
    """(ref64 [K,C], abs64 [K,C], counts [K]): the float64 sums of the exact products and of their absolute values, by
    np.add.at -- nothing of label_sums' code path (no float32 product, no parts, no order)."""
    x = np.asarray(rows).astype(np.float64)
    if row_scale is not None:
        x = x * np.asarray(row_scale).astype(np.float64)[:, None]
    labels = np.asarray(labels, dtype=np.int64)
    keep = (labels >= 0) & (labels < K)
    ref = np.zeros((K, x.shape[1]))
    ab = np.zeros((K, x.shape[1]))
    np.add.at(ref, labels[keep], x[keep])
    np.add.at(ab, labels[keep], np.abs(x[keep]))
    return ref, ab, np.bincount(labels[keep], minlength=K).astype(np.int64)


def inv_norms64(rows):
    """(inv f64 [N], zero bool [N], bad bool [N]): 1 / max(|x|, 1e-12) in float64; 0 for all-zero and non-finite rows."""
    x = np.asarray(rows).astype(np.float64)
    bad = ~np.isfinite(x).all(axis=1)
    x = np.where(bad[:, None], 0.0, x)
    ss = (x * x).sum(axis=1)
    zero = (ss == 0.0) & ~bad
    inv = 1.0 / np.maximum(np.sqrt(ss), 1e-12)
    inv[zero | bad] = 0.0
    return inv, zero, bad


def kmeans64(rows, centroids, max_iter=100):
    """Spherical Lloyd iterations in float64 from ``centroids`` [K,C] on the valid rows of ``rows`` (the others keep label
    -1): dict(centroids, labels, objective, n_iter, history=[(objective, changed), ...]).  The objective of an iteration is
    sum_k S_k . c_k with the centroids that produced its labels; the loop stops when the labels repeat."""
    inv, zero, bad = inv_norms64(rows)
    valid = ~(zero | bad)
    x = np.where(valid[:, None], np.asarray(rows).astype(np.float64), 0.0) * inv[:, None]
    c = np.asarray(centroids, dtype=np.float64)
    c = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)
    K = len(c)
    labels = np.full(len(x), -2, np.int64)
    history = []
    for it in range(max_iter):
        new = (x @ c.T).argmax(axis=1)
        new[~valid] = -1
        changed = int((new != labels).sum())
        if changed == 0:
            break
        labels = new
        S = np.zeros_like(c)
        np.add.at(S, labels[valid], x[valid])
        history.append((float((S * c).sum()), changed))
        norm = np.linalg.norm(S, axis=1, keepdims=True)
        c = np.where(norm > 0, S / np.maximum(norm, 1e-300), c)
    labels = (x @ c.T).argmax(axis=1)
    labels[~valid] = -1
    S = np.zeros_like(c)
    np.add.at(S, labels[valid], x[valid])
    return dict(centroids=c, labels=labels, objective=float((S * c).sum()), n_iter=len(history), history=history, K=K)


def planted_scene(N, C, K, sigma, seed):
    """(rows float16 [N,C], labels int64 [N], directions f64 [K,C]): K planted unit directions, cluster weights uniform in
    [0.3, 1] then normalised, x = (dir + sigma * noise / sqrt(C)) * u with u uniform in [0.5, 4], cast to float16."""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(K, C))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    w = rng.uniform(0.3, 1.0, K)
    labels = rng.choice(K, size=N, p=w / w.sum())
    u = rng.uniform(0.5, 4.0, N)
    x = (dirs[labels] + sigma * rng.normal(size=(N, C)) / np.sqrt(C)) * u[:, None]
    return x.astype(np.float16), labels.astype(np.int64), dirs


def adjusted_rand(a, b):
    """The adjusted Rand index of two labelings (rows with a negative label in either are left out)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    keep = (a >= 0) & (b >= 0)
    a, b = np.unique(a[keep], return_inverse=True)[1], np.unique(b[keep], return_inverse=True)[1]
    n = len(a)
    table = np.zeros((a.max() + 1, b.max() + 1), np.int64)
    np.add.at(table, (a, b), 1)

    def pairs(v):
        v = v.astype(np.float64)
        return (v * (v - 1) / 2).sum()

    s_ab, s_a, s_b = pairs(table.ravel()), pairs(table.sum(1)), pairs(table.sum(0))
    expected = s_a * s_b / (n * (n - 1) / 2)
    return float((s_ab - expected) / ((s_a + s_b) / 2 - expected))


def same_partition(a, b):
    """Whether two labelings are one partition up to a renaming of the ids."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
