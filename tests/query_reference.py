"""The text query's contract in float64 NumPy (shared by test_query_cpu.py and test_gpu_query.py).

x^ = x / max(|x|, 1e-12), t^_j = t_j / max(|t_j|, 1e-12), logit_j = scale * x^ . t^_j, label = argmax (lowest j on ties),
margin = softmax top-1 minus top-2 (1 when P = 1).  bound(C, scale) is the per-logit accuracy B the kernel promises.
"""
import numpy as np


def bound(C, scale=1.0):
    return scale * (2.0 ** -11 + 2 * C * 2.0 ** -24)


def query64(rows, text, scale=1.0):
    """(logits f64 [N,P], labels int64 [N], margin f64 [N], bad bool [N]) of the formula; bad rows (a non-finite element) get
    label -1 and NaN logits / margin."""
    x = np.asarray(rows, dtype=np.float64)
    t = np.asarray(text, dtype=np.float64)
    bad = ~np.isfinite(x).all(axis=1)
    x = np.where(bad[:, None], 0.0, x)
    xn = x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
    tn = t / np.maximum(np.sqrt((t * t).sum(axis=1, keepdims=True)), 1e-12)
    logits = scale * (xn @ tn.T)
    labels = logits.argmax(axis=1)
    P = logits.shape[1]
    if P == 1:
        margin = np.ones(len(x))
    else:
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        ps = np.sort(p, axis=1)
        margin = ps[:, -1] - ps[:, -2]
    logits[bad] = np.nan
    labels[bad] = -1
    margin[bad] = np.nan
    return logits, labels, margin, bad


def check(rows, text, scale, labels, logits=None, margin=None):
    """Assert the kernel's outputs meet the contract against query64; returns the worst logit error over B."""
    L64, lab64, m64, bad = query64(rows, text, scale)
    C = np.asarray(rows).shape[1]
    B = bound(C, scale)
    labels = np.asarray(labels)
    assert np.array_equal(labels[bad], lab64[bad])
    good = ~bad
    Lg = L64[good]
    worst = 0.0
    if logits is not None:
        logits = np.asarray(logits, dtype=np.float64)
        assert np.isnan(logits[bad]).all()
        err = np.abs(logits[good] - Lg)
        worst = float(err.max() / B) if err.size else 0.0
        assert worst <= 1.0, f"logit error {err.max():.3e} above B = {B:.3e}"
    # labels: exact where the top-1/top-2 gap exceeds 2B, else within 2B of the maximum
    lab = labels[good]
    assert (lab >= 0).all() and (lab < L64.shape[1]).all()
    if Lg.size:
        srt = np.sort(Lg, axis=1)
        gap = srt[:, -1] - srt[:, -2] if Lg.shape[1] > 1 else np.full(len(Lg), np.inf)
        clear = gap > 2 * B
        assert np.array_equal(lab[clear], lab64[good][clear]), "label differs where the float64 gap exceeds 2B"
        chosen = Lg[np.arange(len(lab)), lab]
        assert (srt[:, -1] - chosen <= 2 * B).all()
    if margin is not None:
        margin = np.asarray(margin, dtype=np.float64)
        assert np.isnan(margin[bad]).all()
        dm = np.abs(margin[good] - m64[good])
        assert (dm <= 2 * B + 1e-6).all(), f"margin error {dm.max():.3e}"
    return worst


def palette(n):
    """The bit-interleaved label palette (label 1 -> (128,0,0), 2 -> (0,128,0), 8 -> (64,0,0)), uint8 [n,3]; an independent
    re-statement of the rule for the tests: bit 3b + c of the label sets bit 7 - b of channel c."""
    out = np.zeros((n, 3), np.uint8)
    for i in range(n):
        lab, b = i, 0
        c = [0, 0, 0]
        while lab:
            for ch in range(3):
                c[ch] |= ((lab >> ch) & 1) << (7 - b)
            lab >>= 3
            b += 1
        out[i] = c
    return out
