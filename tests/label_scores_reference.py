"""numpy statement of the label-map scores (include/voxproj.h, "Scoring label maps"): the confusion by direct counting, the
boundary band in two independent formulations, the boundary counts class by class, and seeded piecewise-constant maps.
The metric arithmetic is label_metrics.py's (the package's pure host function); hand-checkable values of it are in
test_label_scores_cpu.py.  Everything here is an integer and every comparison against it is exact."""
import numpy as np


def make_map(W, H, P, seed, n_rects=12, n_dots=10, invalid=0.0, invalid_values=(-1, 255)):
    """A piecewise-constant i32 [H,W] map: rectangles of every scale and single pixels over a background, labels in [0, P);
    about ``invalid`` of the area is then overwritten with rectangles of the ``invalid_values``."""
    rng = np.random.default_rng(seed)
    m = np.full((H, W), int(rng.integers(0, P)), np.int32)
    for _ in range(n_rects):
        w, h = int(rng.integers(1, max(2, W // 2 + 1))), int(rng.integers(1, max(2, H // 2 + 1)))
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        m[y:y + h, x:x + w] = int(rng.integers(0, P))
    for _ in range(n_dots):
        m[int(rng.integers(0, H)), int(rng.integers(0, W))] = int(rng.integers(0, P))
    if invalid > 0:
        covered = np.zeros((H, W), bool)
        for _ in range(1000):
            if covered.mean() >= invalid:
                break
            w, h = int(rng.integers(1, max(2, W // 6 + 1))), int(rng.integers(1, max(2, H // 6 + 1)))
            x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
            m[y:y + h, x:x + w] = invalid_values[int(rng.integers(0, len(invalid_values)))]
            covered[y:y + h, x:x + w] = True
    return m


def perturb(m, P, seed, n_rects=6, n_bad=3, bad_values=(-1, 255, 1 << 20)):
    """A prediction for the target ``m``: some rectangles relabelled, and ``n_bad`` small patches of labels outside [0, P)."""
    rng = np.random.default_rng(seed)
    H, W = m.shape
    p = m.copy()
    p[(p < 0) | (p >= P)] = int(rng.integers(0, P))          # a prediction is mostly valid where the target is not
    for _ in range(n_rects):
        w, h = int(rng.integers(1, max(2, W // 3 + 1))), int(rng.integers(1, max(2, H // 3 + 1)))
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        p[y:y + h, x:x + w] = int(rng.integers(0, P))
    for k in range(n_bad):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        p[y:y + 2, x:x + 3] = bad_values[k % len(bad_values)]
    return p


def confusion(pred, target, P):
    """(confusion i64 [P,P] with rows = ground truth, skipped i64 [2]) by direct counting."""
    pred, target = np.asarray(pred).astype(np.int64).ravel(), np.asarray(target).astype(np.int64).ravel()
    conf, skipped = np.zeros((P, P), np.int64), np.zeros(2, np.int64)
    for p, t in zip(pred.tolist(), target.tolist()):
        if not 0 <= t < P:
            skipped[0] += 1
        elif not 0 <= p < P:
            skipped[1] += 1
        else:
            conf[t, p] += 1
    return conf, skipped


def erode3x3(mask):
    """One 3x3 minimum of a boolean mask; what lies outside the array counts as 0.  (The minimum over a 3x3 square is the
    minimum over three columns of the minimum over three rows.)"""
    rows = np.zeros_like(mask)
    rows[:, 1:-1] = mask[:, 1:-1] & mask[:, :-2] & mask[:, 2:]
    out = np.zeros_like(mask)
    out[1:-1] = rows[1:-1] & rows[:-2] & rows[2:]
    return out


def mask_boundary(mask, r):
    """Formulation (a) for one binary mask: pad one pixel of zeros, erode r times with a 3x3 minimum, mask - eroded."""
    H, W = mask.shape
    padded = np.zeros((H + 2, W + 2), bool)
    padded[1:-1, 1:-1] = mask
    er = padded
    for _ in range(r):
        er = erode3x3(er)
        if not er.any():                                        # nothing left: further erosions change nothing
            break
    return mask & ~er[1:-1, 1:-1]


def band_by_erosion(labels, r):
    """Formulation (a): the union over every label value present of its mask's boundary.  u8 [H,W]."""
    labels = np.asarray(labels)
    band = np.zeros(labels.shape, bool)
    for c in np.unique(labels):
        band |= mask_boundary(labels == c, r)
    return band.astype(np.uint8)


def band_by_window(labels, r):
    """Formulation (b): band = 1 iff some pixel of the (2r+1)^2 window lies outside the image or differs from the centre, by
    shifted comparisons against a map padded by r with a sentinel no label equals.  The window holds the centre's label only
    iff every row of it does (shifts along x give row_same) and every row's centre equals the centre (shifts along y).
    u8 [H,W]."""
    H, W = np.asarray(labels).shape
    # equality is all that matters: the labels as their ranks among the values present (>= 0), the sentinel -1
    lab = np.unique(np.asarray(labels), return_inverse=True)[1].reshape(H, W).astype(np.int32)
    sentinel = -1
    padx = np.full((H, W + 2 * r), sentinel, np.int32)
    padx[:, r:r + W] = lab
    row_same = np.ones((H, W), bool)           # labels[y, x - r .. x + r] lie in the image and equal labels[y, x]
    for d in range(1, r + 1):
        row_same &= (padx[:, r - d:r - d + W] == lab) & (padx[:, r + d:r + d + W] == lab)
    pady = np.full((H + 2 * r, W), sentinel, np.int32)
    pady[r:r + H] = lab
    rows = np.zeros((H + 2 * r, W), bool)      # row_same, False outside the image
    rows[r:r + H] = row_same
    same = row_same.copy()
    for d in range(1, r + 1):
        same &= rows[r - d:r - d + H] & (pady[r - d:r - d + H] == lab) & rows[r + d:r + d + H] & (pady[r + d:r + d + H] == lab)
    return (~same).astype(np.uint8)


def sparse_map(W, H, r, background=2):
    """A map for a large radius r: one background label and three small features (top right, bottom left, centre), so that
    pixels outside the band exist wherever W and H leave room for them, next to pixels inside it."""
    m = np.full((H, W), background, np.int32)
    m[min(H - 1, r // 4), max(0, W - 1 - r // 3)] = 1
    m[max(0, H - 2 - r // 5):max(1, H - r // 5), r // 2:r // 2 + 3] = 3
    m[H // 2, W // 2] = -1
    return m


def boundary_counts_from_bands(pred, target, P, pband, tband):
    """(bnd_inter, bnd_union) from two given bands, by the definition in the header."""
    pred, target = np.asarray(pred), np.asarray(target)
    valid = (target >= 0) & (target < P)
    pb, tb = np.asarray(pband).astype(bool), np.asarray(tband).astype(bool)
    inter, union = np.zeros(P, np.int64), np.zeros(P, np.int64)
    for c in range(P):
        a, b = (pred == c) & pb, (target == c) & tb
        inter[c] = int((a & b & valid).sum())
        union[c] = int(((a | b) & valid).sum())
    return inter, union


def boundary_counts(pred, target, P, r):
    """(bnd_inter i64 [P], bnd_union i64 [P]) class by class from formulation (a), over the pixels with a valid target."""
    pred, target = np.asarray(pred), np.asarray(target)
    valid = (target >= 0) & (target < P)
    inter, union = np.zeros(P, np.int64), np.zeros(P, np.int64)
    for c in range(P):
        pb = mask_boundary(pred == c, r)
        tb = mask_boundary(target == c, r)
        inter[c] = int((pb & tb & valid).sum())
        union[c] = int(((pb | tb) & valid).sum())
    return inter, union


def nearest_resize(src, W, H):
    """Nearest-neighbour resample to [H,W] with src = floor((dst + 0.5) * src_size / dst_size)."""
    src = np.asarray(src)
    h, w = src.shape
    ys = np.minimum(np.floor((np.arange(H) + 0.5) * h / H).astype(np.int64), h - 1)
    xs = np.minimum(np.floor((np.arange(W) + 0.5) * w / W).astype(np.int64), w - 1)
    return src[ys][:, xs]
