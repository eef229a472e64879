"""The order of the fixed-order float64 sums, bit for bit: for every loss family whose statistics are a two-step sum of
per-element float32 terms (csrc/vp_reduce.h: a halving tree over a workgroup's slots, then the workgroups in ascending index),
the statistics a call returns equal, byte for byte, the numpy twin of tests/sum_order.py applied to the per-element outputs
of that same call.

A float64 sum of float32 terms of similar size is exact in any order, so a comparison inside a bound, or of two runs, cannot
see the order change.  Here the terms are spread over about 40 binades (weights or values 2^uniform(-20, 20) times a value in
[0.2, 2]), and every case whose order differs from a plain loop asserts, on the device's own terms, that the twin's bits
differ from the plain ascending float64 sum of the same terms: the comparison can fail.  Cases with one term, or with one
term per workgroup (feature loss 1 x 1, neighbour KL S = 1 and 255), are left-to-right sums by construction: they check the
zero slots and the empty workgroups, not the order.

Thread-to-element maps, as read from the kernels:
  splat loss     k_splat_blend<DT, true>: workgroup = 16 x 16 tile, tiles row-major; slot 16 ty + tx = pixel (tx, ty) of the
                 tile; a pixel outside the image holds (0, 0); a pixel whose target is outside [0, D) has weight 0.
  feature loss   k_feature_loss: workgroup b, slot t = pixel 256 b + t of the row-major image; m = weight, or 0 where
                 alpha < min_alpha.
  photo loss     k_photo_loss: workgroup = 32 x 32 tile of one plane, in ascending (c, tile row, tile); slot 32 ty + tx.
                 |x - y| and (x - y)^2 are one fp32 subtraction, fabsf, one fp32 product (no contraction): numpy float32 gives
                 the same bits.  sum m: the terms lie in [-1, 1] and add exactly in any order, so the visibility assertion
                 covers the other two components only.
  neighbour KL   k_kl_sum1 / k_kl_sum2: 256 workgroups over per = ceil(S / 256) consecutive samples each; slot t of a
                 workgroup = its samples t, t + 256, .. added in that order; the tree; then the 256 totals in ascending order.
The prototype and code-book statistics accumulate per thread over grid-strided tiles before the tree: no twin here."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "3d-semantic-segmentation_amd")
for p in (HERE, ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import sum_order as so  # noqa: E402
import voxproj_host  # noqa: E402
from test_gpu_splat import camera, scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def spread(rng, shape):
    """float32 values 2^uniform(-20, 20) times a value in [0.2, 2]"""
    return (np.exp2(rng.uniform(-20.0, 20.0, shape)) * rng.uniform(0.2, 2.0, shape)).astype(np.float32)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(name, got, slots_of, terms, threads, visible):
    """got: the call's float64 statistics; terms: one per-element float32 array per statistic; slots_of(terms[i]) the
    workgroups' slots.  Byte equality with the twin, and for the statistics listed in ``visible`` other bytes than the plain
    ascending sum of the same terms."""
    got = np.asarray(got, np.float64)
    for i, t in enumerate(terms):
        twin, plain = so.two_step(slots_of(t), threads), so.ascending(t)
        print(f"sum-order {name}[{i}]: device {got[i]!r} twin {twin!r} ascending {plain!r}", flush=True)
        assert so.bits(got[i]) == so.bits(twin), f"{name}[{i}]: device {got[i]!r} is not the twin's {twin!r}"
        if i in visible:
            assert so.bits(twin) != so.bits(plain), f"{name}[{i}]: the order is not visible in this case: reshape it"


@pytest.mark.parametrize("W,H", [(37, 19), (685, 107)])
def test_splat_loss(W, H):
    """37 x 19: six tiles with both tails.  685 x 107: 43 x 7 = 301 tiles, a second staging lap of the ordered sum."""
    D = 13
    s = {k: to_dev(v) for k, v in scene(400, D, 13).items()}
    vm, K = camera(W, H)
    rng = np.random.default_rng(W)
    target = rng.integers(0, D, (H, W)).astype(np.int32)
    u = rng.uniform(size=(H, W))
    target[u < 0.05] = -1
    target[(u >= 0.05) & (u < 0.1)] = D + 3
    w = spread(rng, (H, W))
    r = voxproj_host.splat_loss(s["means"], s["quats"], s["scales"], s["opacities"], s["features"], vm, K, W, H, to_dev(target),
                                to_dev(w), want_pixel_loss=True, check=False)
    torch.cuda.synchronize()
    wl = r.pixel_loss.cpu().numpy()
    m = np.where((target >= 0) & (target < D), w, np.float32(0.0))
    assert (wl[m == 0] == 0).all() and (wl[m != 0] != 0).mean() > 0.99
    check(f"splat {W}x{H}", r.loss_stats.cpu().numpy(), lambda t: so.tile_slots(t, 16), [wl, m], 256, {0, 1})


@pytest.mark.parametrize("W,H", [(1, 1), (37, 19), (257, 256)])
def test_feature_loss(W, H):
    """1 x 1: one slot of one workgroup.  37 x 19: three workgroups, the last with a tail of zero slots.  257 x 256: 257
    workgroups, a second staging lap of the ordered sum."""
    C, min_alpha = 8, 0.5
    rng = np.random.default_rng(1000 + W)
    image = rng.normal(size=(H, W, C)).astype(np.float32)
    target = rng.normal(size=(H, W, C)).astype(np.float16)
    assert (np.abs(image).max(-1) > 0).all() and (np.abs(target.astype(np.float32)).max(-1) > 0).all()
    w = spread(rng, (H, W))
    alpha = np.where(rng.uniform(size=(H, W)) < 0.1, 0.25, 0.75).astype(np.float32)     # clearly below / above min_alpha
    if W * H == 1:
        alpha[:] = 0.75
    stats, pl, _ = voxproj_host.feature_loss(to_dev(image), to_dev(target), to_dev(w), to_dev(alpha), kind="cosine",
                                             min_alpha=min_alpha, want_pixel_loss=True)
    torch.cuda.synchronize()
    ml = pl.cpu().numpy()
    m = np.where(alpha >= min_alpha, w, np.float32(0.0))
    assert (ml[m == 0] == 0).all() and (ml[m != 0] != 0).all()
    check(f"feature {W}x{H}", stats.cpu().numpy(), lambda t: so.chunk_slots(t, 256), [ml, m], 256,
          {0, 1} if W * H > 256 else set())


@pytest.mark.parametrize("C,W,H", [(1, 33, 31), (3, 1051, 349)])
def test_photo_loss(C, W, H):
    """33 x 31: two tiles, the second one column wide.  C = 3, 1051 x 349: 3 x 11 x 33 = 1089 tiles, a second staging lap.
    The one-workgroup evaluation path (no workspace) must give the same bytes."""
    rng = np.random.default_rng(C * 7 + W)
    x = (spread(rng, (C, H, W)) * rng.choice(np.float32([-1.0, 1.0]), (C, H, W))).astype(np.float32)
    y = (x * rng.uniform(0.3, 0.7, (C, H, W)).astype(np.float32)).astype(np.float32)
    xt, yt = to_dev(x), to_dev(y)
    stats, ssim, _ = voxproj_host.photo_loss(xt, yt, want_ssim_map=True)
    stats_e, ssim_e, _ = voxproj_host.photo_loss(xt, yt, want_ssim_map=True, evaluate_only=True)
    torch.cuda.synchronize()
    d = x - y
    assert d.dtype == np.float32
    mm = ssim.cpu().numpy()
    assert np.isfinite(mm).all() and np.abs(mm).max() <= 1.0 + 1e-3
    assert mm.tobytes() == ssim_e.cpu().numpy().tobytes()

    def slots(t):
        return np.concatenate([so.tile_slots(t[c], 32) for c in range(C)])
    got = stats.cpu().numpy()
    check(f"photo {C}x{W}x{H}", got, slots, [np.abs(d), d * d, mm], 1024, {0, 1})
    assert got.tobytes() == stats_e.cpu().numpy().tobytes(), "evaluate_only gives other bytes"


KL_SEED = 0


def kl_twin(sl):
    """k_kl_sum1 / k_kl_sum2 on the per-sample losses"""
    S = len(sl)
    per = -(-S // 256)
    laps = -(-per // 256)
    p = np.zeros((256, laps * 256), np.float64)
    flat = np.zeros(256 * per, np.float64)
    flat[:S] = sl
    p[:, :per] = flat.reshape(256, per)
    slot = np.zeros((256, 256), np.float64)
    for lap in range(laps):                                 # a thread's samples t, t + 256, .. in that order
        slot = slot + p[:, 256 * lap:256 * (lap + 1)]
    return so.ordered(so.tree_sum(slot, 256))


@pytest.mark.parametrize("S", [1, 255, 257, 65837])
def test_neighbor_kl(S):
    """S = 1, 255: one sample per workgroup, the sum is left to right.  S = 257: per = 2, 129 workgroups of two slots (the last
    of one), 127 empty ones.  S = 65837: per = 258, threads 0 and 1 of a workgroup take a second lap."""
    N, P, k = 600, 4, 5
    rng = np.random.default_rng(KL_SEED + S)
    # Rows in pairs (a, 0, 0, 0), (a + 1, 0, 0, 0), a uniform in [1, 30]; a sample's four neighbours are all its row's partner.
    # Beyond a few units the divergence is 3 e^-a (1 - e^-1) to first order, every product of it small on its own and none
    # the rest of a cancellation: the per-sample losses keep their 24 bits from 2^0 down to 2^-43.
    a = rng.uniform(1.0, 30.0, N // 2)
    logits = np.zeros((N, P), np.float32)
    logits[0::2, 0] = a
    logits[1::2, 0] = a + 1.0
    # The samples in ascending a, the large losses first: the running sum has its final magnitude when the small ones arrive,
    # so a rounding that differs between the orders is not rounded away again by a later large term.
    samples = rng.integers(0, N, S)
    samples = samples[np.argsort(logits[samples, 0], kind="stable")].astype(np.int32)
    nbr = np.repeat((samples ^ 1)[:, None], k - 1, 1).astype(np.int32)
    ns = voxproj_host.NeighborSample(N, k, to_dev(samples), to_dev(nbr))
    stats, _, sl, _ = voxproj_host.neighbor_kl(to_dev(logits), ns, want_sample_loss=True)
    torch.cuda.synchronize()
    sl, got = sl.cpu().numpy(), stats.cpu().numpy()
    assert np.isfinite(sl).all() and (sl != 0).mean() > 0.9
    twin, plain = kl_twin(sl), so.ascending(sl)
    print(f"sum-order kl S={S}: device {got[0]!r} twin {twin!r} ascending {plain!r}", flush=True)
    assert so.bits(got[0]) == so.bits(twin), f"device {got[0]!r} is not the twin's {twin!r}"
    assert got[1] == S
    if S > 256:
        assert so.bits(twin) != so.bits(plain), "the order is not visible in this case: reshape it"
