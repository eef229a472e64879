"""The projector's transpose on every path its host code can select, each against a reference computed without the library
(NumPy, or the CPU oracle's first-hit image).  Lines are csrc/voxproj.hip unless another file is named.

  A  vp_render_features (voxproj.hip:551-578): dst[p] = rows[ids[p]] for 0 < ids[p] < n_rows, zeros otherwise; the bad IDs
     counted.  Six instantiations, chosen by C, the dtype and al16 = rows and dst both 16-byte aligned (:559):
       k_render_small<float>          C < 64 (:572)                     k_render_small<_Float16>       C < 64 (:567)
       k_render_walk<4,2,float>       C % 4 == 0 && al16 (:573)         k_render_walk<8,1,_Float16>    C % 8 == 0 && al16 (:568)
       k_render_walk<1,4,float>       otherwise (:574)                  k_render_walk<1,4,_Float16>    otherwise (:569)
     A pass of the walk (vp_render.h:82) is 64*VEC*K channels: 512 for <4,2> and <8,1>, 256 for <1,4>.  Bit for bit against
     np.where(ids > 0, rows[ids], 0) (fp16: its .astype(np.float16), round-to-nearest-even), at every width class, with rows
     and dst off 16-byte alignment, at pixel counts around a tile of 64, on ID streams built to break the walk's register
     reuse (vp_render.h:94-115: a row is kept while the ID repeats, compared across groups of RENDER_UNR = 4 pixels).  dst lies
     between guard words: no byte outside it is written.
  B  past the grid cap (RENDER_MAX_BLOCKS = 2^20 blocks of 4 tiles, :547,558): 2^28 + 837 pixels, so blocks 0-3 take a second
     tile in the grid-stride loop (vp_render.h:78,153) and the last tile holds 5 pixels.
  C  vp_first_hit_ids (voxproj.hip; project_march of vp_project.h without a plan or a work list): batched calls with a different grid per
     batch, up to 70 views, both march modes, against the oracle's hit image; then on a workspace whose pipelined forward
     calls (VP_FLAG_PIPELINE) are still in flight.
  D  project_features_autograd.ProjectFeatures: the gradient against g[oracle_hits] ("sum") or g / max(oracle_count, 1)
     ("mean"), the forward out against the oracle by tests/sum_criteria.py.
"""
import ctypes

import numpy as np
import pytest
import torch

from sum_criteria import abs_sums_from_hits, assert_sums, assert_sums_vs_oracle
from synthetic_scene import make_features_np, make_scene
from test_gpu_kernel_variants import _guards_intact, _offset_empty
from test_gpu_parity import _random_rotation
from test_gpu_render import _oracle_hits, _same_f16, _special_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = -7.0
FILL = 12345.0                   # what dst holds before the render: every element must be overwritten


# ------------------------------------------------------------------------------------------------------------------------------
# A. vp_render_features, every instantiation
# ------------------------------------------------------------------------------------------------------------------------------
def _bad_ids(rng, n_rows, k):
    return rng.choice(np.array([-1, -2, n_rows, n_rows + 5, -(2 ** 31), 2 ** 31 - 1], np.int64), k).astype(np.int32)


def _reuse_stream(n_rows, seed):
    """An ID stream (int32, ~2800 pixels) of segments that each break one rule of the walk's register reuse: runs of 1 to 9
    pixels and of 63 to 130 (they cross groups of 4, tiles of 64 and the following pass's first pixel), A-B-A, X-0-X and X-bad-X
    at every phase of a group of 4, a run of one ID and a run of misses.  IDs are 1..n_rows-1 except where stated."""
    rng = np.random.default_rng(seed)
    ids = lambda k: rng.integers(1, n_rows, k).astype(np.int32)     # noqa: E731
    seg = []
    for ln in list(range(1, 10)) * 6:
        seg.append(np.full(ln, ids(1)[0] if rng.random() < 0.85 else 0, np.int32))
    for ln in list(range(63, 131, 5)) + [64, 65, 128, 129]:
        seg.append(np.full(ln, ids(1)[0], np.int32))
    for phase in range(8):
        seg.append(ids(phase + 1))                                    # shifts the pattern by one pixel each time
        a, b, x = ids(3)
        seg.append(np.array([a, b, a, b, a, a, b, a], np.int32))
        seg.append(np.array([x, 0, x, 0, 0, x, x, 0, x], np.int32))
        seg.append(np.array([x, _bad_ids(rng, n_rows, 1)[0], x, x, _bad_ids(rng, n_rows, 1)[0], _bad_ids(rng, n_rows, 1)[0], x], np.int32))
    seg.append(np.full(200, ids(1)[0], np.int32))
    seg.append(np.zeros(150, np.int32))
    for _ in range(40):                                               # a row that returns after one other pixel, across groups
        a, b = ids(2)
        seg.append(np.array([a] * int(rng.integers(1, 6)) + [b] + [a] * int(rng.integers(1, 6)), np.int32))
    return np.concatenate(seg)


def _want(ids, rows, f16):
    n_rows = rows.shape[0]
    ok = (ids > 0) & (ids < n_rows)
    want = np.where(ok[:, None], rows[np.where(ok, ids, 0)], np.float32(0))
    if f16:
        with np.errstate(over="ignore"):               # 7e4 rounds to inf in float16, as it should
            want = want.astype(np.float16)
    return want, int(((ids < 0) | (ids >= n_rows)).sum())


def _render_raw(ids_t, rows_t, dst_t, f16, bad_t):
    import voxproj_host as vh
    C = int(rows_t.shape[1])
    vh.check(vh.lib().vp_render_features(ids_t.data_ptr(), ids_t.numel(), rows_t.data_ptr(), int(rows_t.shape[0]), C,
                                         dst_t.data_ptr(), int(f16), bad_t.data_ptr() if bad_t is not None else None,
                                         ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))


def _check_render(ids, rows, rows_off, dst_off, f16):
    """One vp_render_features call on int32 ``ids`` and float32 ``rows`` placed ``rows_off`` / ``dst_off`` elements into their
    allocations; dst between guard words, prefilled with FILL.  Asserts the bits, the bad-ID count and the guards."""
    n, (n_rows, C) = ids.size, rows.shape
    rows_t, _ = _offset_empty((n_rows, C), torch.float32, rows_off)
    rows_t.copy_(torch.from_numpy(rows))
    dt = torch.float16 if f16 else torch.float32
    dst, buf = _offset_empty((n, C), dt, dst_off, fill=FILL, guard=GUARD)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _render_raw(torch.from_numpy(ids).to(DEV), rows_t, dst, f16, bad)
    torch.cuda.synchronize()
    want, n_bad = _want(ids, rows, f16)
    got = dst.cpu().numpy()
    where = f"n={n} C={C} f16={f16} rows_off={rows_off} dst_off={dst_off}"
    if f16:
        assert _same_f16(got, want), where
    else:
        assert got.tobytes() == want.tobytes(), (where, int((got.view(np.int32) != want.view(np.int32)).sum()))
    assert int(bad.item()) == n_bad, where
    assert _guards_intact(dst, buf, GUARD), where


def _streams(n_rows, seed):
    s = _reuse_stream(n_rows, seed)
    rng = np.random.default_rng(seed + 1)
    out = [s, np.full(257, int(rng.integers(1, n_rows)), np.int32), np.zeros(130, np.int32)]
    for n in (1, 63, 64, 65, 127, 4 * 33 + 3, 1001):                   # pixel counts around a tile; 1001 = 4k + 1
        out.append(s[int(rng.integers(0, s.size - n)):][:n].copy())
    return out


ALIGN = [(0, 0), (1, 0), (0, 1), (1, 1)]   # (rows, dst) offsets in elements: 4 bytes (fp32) / 2 bytes (fp16 dst) off 16


@pytest.mark.parametrize("C", range(1, 64))
def test_render_small_every_width(C):
    """k_render_small<float> and <_Float16> (voxproj.hip:572,567: C < 64, any alignment) at every C it takes."""
    n_rows = 97
    rows = _special_rows(n_rows, C, seed=1000 + C)
    for i, ids in enumerate(_streams(n_rows, seed=C)):
        for f16 in (False, True):
            for ro, do in (ALIGN if i == 0 else ALIGN[:1] + ALIGN[3:]):
                _check_render(ids, rows, ro, do, f16)


# (C, dtype is f16, alignments): the instantiation each alignment reaches is in the docstring of the test
WALK_CASES = ([(C, False, "4,2 | 1,4") for C in (64, 516, 1024, 1028)] + [(C, False, "1,4") for C in (67, 255, 257, 513, 1001)]
              + [(C, True, "8,1 | 1,4") for C in (520, 1024)] + [(C, True, "1,4") for C in (68, 100, 67, 255, 257, 513, 1001)])


@pytest.mark.parametrize("C,f16,kernels", WALK_CASES)
def test_render_walk_every_width_and_alignment(C, f16, kernels):
    """The walk.  fp32: C % 4 == 0 aligned -> k_render_walk<4,2,float> (voxproj.hip:573; C = 64, 516, 1024, 1028: one to three
    passes of 512, the last partial); rows or dst 4 bytes off, or C % 4 != 0 -> <1,4,float> (:574; passes of 256: C = 67 one
    partial, 255 one, 257 two, 513 three, 1001 four).  fp16: C % 8 == 0 aligned -> <8,1,_Float16> (:568; C = 520 two passes,
    1024 two); misaligned, or C % 8 != 0 (68, 100: C % 4 == 0; the odd widths) -> <1,4,_Float16> (:569)."""
    n_rows = 53
    rows = _special_rows(n_rows, C, seed=2000 + C + f16)
    for i, ids in enumerate(_streams(n_rows, seed=C + 7 * f16)):
        for ro, do in (ALIGN if i < 3 else ALIGN[:1] + ALIGN[3:]):
            _check_render(ids, rows, ro, do, f16)


@pytest.mark.parametrize("C,f16", [(5, False), (40, True), (64, False), (100, False), (1024, True), (100, True)])
def test_render_counts_thousands_of_bad_ids_over_many_wavefronts(C, f16):
    """The bad-ID counter (vp_render.h:61-66: one atomic per wavefront that saw any) of every instantiation: ~12 000 IDs outside
    [0, n_rows) spread over 3 900 tiles, each rendering zeros; the count equals NumPy's."""
    rng = np.random.default_rng(C + f16)
    n_rows, n = 211, 250_003
    ids = rng.integers(0, n_rows, n).astype(np.int32)
    pick = rng.random(n) < 0.05
    ids[pick] = _bad_ids(rng, n_rows, int(pick.sum()))
    rows = _special_rows(n_rows, C, seed=C)
    for ro, do in ALIGN[:1] + ALIGN[3:]:
        _check_render(ids, rows, ro, do, f16)


# ------------------------------------------------------------------------------------------------------------------------------
# B. Past the grid cap
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,f16", [(1, False), (3, False), (1, True), (3, True), (64, True)])
def test_render_past_the_grid_cap_takes_a_second_tile(C, f16):
    """2^28 + 837 pixels: the grid is capped at 2^20 blocks x 4 tiles x 64 pixels = 2^28 pixels (voxproj.hip:558), so the
    grid-stride loop (vp_render.h:78,153) gives 14 more tiles to blocks 0-3, the last of 5 pixels.  k_render_small<float>,
    <_Float16> (C = 1, 3) and k_render_walk<8,1,_Float16> (C = 64: 34 GB of dst).  Checked in chunks against a torch gather;
    two bad IDs in the second-pass tiles are counted."""
    n_pix, n_rows = 2 ** 28 + 800 + 37, 100_003
    tail = 2 ** 28
    g = torch.Generator(device=DEV).manual_seed(C + f16)
    runs = torch.randint(0, n_rows, (n_pix // 7 + 1,), device=DEV, dtype=torch.int32, generator=g)
    ids = runs.repeat_interleave(7)[:n_pix].contiguous()
    del runs
    ids[tail + 3] = -1
    ids[n_pix - 1] = n_rows
    rows = torch.randn(n_rows, C, device=DEV, generator=g)
    dt = torch.float16 if f16 else torch.float32
    dst = torch.empty((n_pix, C), dtype=dt, device=DEV)
    dst[tail - 4096:].fill_(float("nan"))                      # the pixels of the second pass hold NaN until rendered
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _render_raw(ids, rows, dst, f16, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 2
    iv = torch.int16 if f16 else torch.int32
    step = 1 << 22
    zero = torch.zeros((), device=DEV)
    for p0 in range(0, n_pix, step):
        i = ids[p0:p0 + step].long()
        ok = (i > 0) & (i < n_rows)
        ref = torch.where(ok[:, None], rows[torch.where(ok, i, 0)], zero).to(dt)
        assert torch.equal(dst[p0:p0 + step].view(iv), ref.view(iv)), p0
        del i, ok, ref
    del dst, ids, rows, bad
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# C. vp_first_hit_ids against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def _random_job(rng, B=None, V=None):
    """Batched grids (a different occupancy per batch, IDs drawn from one range), cameras inside and around them."""
    B = int(rng.integers(1, 4)) if B is None else B
    dims = rng.integers(4, 28, 3)
    n_ids = int(rng.integers(5, 400))
    occ = np.zeros((B, *dims), np.int64)
    for b in range(B):
        n = min(n_ids, int(occ[b].size * float(rng.uniform(0.01, 0.3))) + 1)
        idx = rng.choice(occ[b].size, n, replace=False)
        occ[b].reshape(-1)[idx] = rng.choice(n_ids, n, replace=False) + 1
    vs = float(np.float32(rng.uniform(0.05, 0.3)))
    origin = rng.uniform(-1, 1, 3).astype(np.float32)
    ext = dims[::-1] * vs
    W, H = int(rng.integers(4, 36)), int(rng.integers(4, 28))
    V = int(rng.choice([1, 2, 5, 17, 70])) if V is None else V
    c2w = np.zeros((B, V, 4, 4), np.float32)
    for b in range(B):
        for v in range(V):
            c2w[b, v, :3, :3] = _random_rotation(rng)
            c2w[b, v, :3, 3] = origin + rng.uniform(-0.3, 1.3, 3) * ext
            c2w[b, v, 3, 3] = 1
    f = float(rng.uniform(0.5, 2.0)) * W
    intr = np.stack([np.array([f, f, W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7)], np.float32) for _ in range(B)])
    opts = np.array([W, H, 0.01, float(2.0 * np.linalg.norm(ext)), float(np.float32(vs * rng.uniform(0.3, 1.2)))], np.float32)
    return dict(occ=occ, c2w=c2w, intr=intr, opts=opts, origin=origin, vs=vs, n_rows=n_ids + 1, B=B, V=V, H=H, W=W)


def _job_tensors(j):
    return (torch.from_numpy(j["occ"]).to(DEV), torch.from_numpy(j["c2w"]).reshape(-1).to(DEV), torch.from_numpy(j["intr"]).to(DEV))


def _job_hits(oracle_mod, j):
    return _oracle_hits(oracle_mod, j["occ"], j["c2w"].reshape(-1), j["intr"], j["opts"], j["origin"], j["vs"], j["B"], j["V"],
                        j["H"], j["W"], j["n_rows"])


def test_first_hit_ids_randomized_batched_differential(oracle_mod):
    """40 random batched configurations (B = 1..3 with a different grid per batch, V up to 70: more than one lane batch of
    views; the first two B*V = 1, the one-view plan), each in both march modes (VP_FLAG_EXACT_MARCH), on one workspace that
    grows and rebuilds its tables as the grids change: the image equals the oracle's hit image exactly."""
    import voxproj_host as vh
    rng = np.random.default_rng(4242)
    ws = vh.Workspace()
    n_hit, n_multi_batch, n_many_views = 0, 0, 0
    for case in range(40):
        j = _random_job(rng, *((1, 1) if case < 2 else (None, None)))
        want = _job_hits(oracle_mod, j)
        occ, vmi, intr = _job_tensors(j)
        for exact in (False, True):
            got = vh.first_hit_ids(occ, vmi, intr, [float(x) for x in j["opts"]], [float(x) for x in j["origin"]], j["vs"], j["H"],
                                   j["W"], j["n_rows"], workspace=ws, exact_march=exact)
            assert tuple(got.shape) == (j["B"], j["V"], j["H"], j["W"])
            assert np.array_equal(got.cpu().numpy(), want), (case, exact, int((got.cpu().numpy() != want).sum()))
        n_hit += bool((want > 0).any())
        n_multi_batch += j["B"] > 1 and not np.array_equal(j["occ"][0], j["occ"][-1])
        n_many_views += j["V"] > 64
    ws.release()
    assert n_hit >= 30 and n_multi_batch >= 15 and n_many_views >= 4, (n_hit, n_multi_batch, n_many_views)


def test_first_hit_ids_between_pipelined_calls_on_one_workspace(oracle_mod):
    """One Workspace: two pipelined forward calls left in flight, vp_first_hit_ids on their grid (tables reused) and on another
    grid (tables rebuilt), one more pipelined call on the first grid.  Both ID images, the last call's hit image and the three
    calls' accumulated counts equal the oracle's; the sums meet tests/sum_criteria.py (heavy threshold 6: voxels split)."""
    import voxproj_host as vh
    rng = np.random.default_rng(99)
    ja = _random_job(rng, B=2, V=17)
    jb = _random_job(rng, B=3, V=5)
    n_rows, B, V, H, W, C = ja["n_rows"], ja["B"], ja["V"], ja["H"], ja["W"], 40
    occ_a, _, intr_a = _job_tensors(ja)
    occ_b, vmi_b, intr_b = _job_tensors(jb)
    opts, origin = [float(x) for x in ja["opts"]], [float(x) for x in ja["origin"]]
    ws = vh.Workspace()
    ws.set_option(vh.VP_OPT_HEAVY_THRESHOLD, 6)
    count = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    out = torch.zeros(n_rows, C, device=DEV)
    calls = []
    for k in range(3):
        c2w = ja["c2w"] if k == 0 else np.stack([[np.eye(4, dtype=np.float32)] * V] * B)
        if k:
            for b in range(B):
                for v in range(V):
                    c2w[b, v, :3, :3] = _random_rotation(rng)
                    c2w[b, v, :3, 3] = ja["origin"] + rng.uniform(-0.3, 1.3, 3) * (ja["occ"].shape[:0:-1] * np.array(ja["vs"]))
        feats = rng.standard_normal((B, V, H, W, C)).astype(np.float32)
        calls.append((torch.from_numpy(feats).to(DEV), torch.from_numpy(np.ascontiguousarray(c2w)).reshape(-1).to(DEV), feats, c2w))
    # two pipelined calls, unsynchronised
    for ft, vm, _, _ in calls[:2]:
        vh.project_features_raw(ft, occ_a, vm, intr_a, opts, count, out, origin, ja["vs"], workspace=ws, pipeline=True)
    ja1 = dict(ja, c2w=calls[1][3])
    ids_a = vh.first_hit_ids(occ_a, calls[1][1], intr_a, opts, origin, ja["vs"], H, W, n_rows, workspace=ws)
    ids_b = vh.first_hit_ids(occ_b, vmi_b, intr_b, [float(x) for x in jb["opts"]], [float(x) for x in jb["origin"]], jb["vs"],
                             jb["H"], jb["W"], jb["n_rows"], workspace=ws)
    vh.project_features_raw(calls[2][0], occ_a, calls[2][1], intr_a, opts, count, out, origin, ja["vs"], workspace=ws, pipeline=True)
    vh.workspace_status(ws, DEV)
    assert np.array_equal(ids_a.cpu().numpy(), _job_hits(oracle_mod, ja1))
    assert np.array_equal(ids_b.cpu().numpy(), _job_hits(oracle_mod, jb))
    # the oracle, call by call, accumulating like the library
    ref_c, ref_o = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32)
    ref64, abs64 = torch.zeros(n_rows, C, dtype=torch.float64, device=DEV), torch.zeros(n_rows, C, dtype=torch.float64, device=DEV)
    for _, _, feats, c2w in calls:
        r = oracle_mod.project_features(feats, ja["occ"], c2w.reshape(-1), ja["intr"], ja["opts"], ja["origin"], ja["vs"], ref_c,
                                        ref_o, want_f64=True)
        assert r["rc"] == 0
        ref64 += torch.from_numpy(r["out64"]).to(DEV)
        abs64 += abs_sums_from_hits(r["hits"].reshape(-1, H, W), feats.reshape(-1, H, W, C), n_rows, DEV)[1]
    assert np.array_equal(vh.hit_image(ws, DEV).cpu().numpy(), r["hits"])
    assert np.array_equal(count.cpu().numpy(), ref_c)
    assert (ref_c > 6).sum() > 10
    assert_sums(out, ref64, abs64, ref_c, split=ref_c > 6, oracle32=ref_o, dev=str(DEV))
    ws.release()


# ------------------------------------------------------------------------------------------------------------------------------
# D. The autograd Function against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def _grad_ref(hits, count, g, reduce, f16):
    """(reference gradient [..., C], tolerance or None for bit-exact): g[hits] for "sum" (zeros where hits == 0), rounded to
    float16 when f16; for "mean" the float64 quotient g[hits] / max(count[hits], 1) and its allowance: one float32 ulp, plus
    half a float16 ulp when the gradient is float16."""
    hit = hits > 0
    rows = np.where(hit[..., None], g[hits], np.float32(0))
    if reduce == "sum":
        return (rows.astype(np.float16) if f16 else rows), None
    q = rows.astype(np.float64) / np.maximum(count[hits], 1)[..., None]
    tol = np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
    if f16:
        tol += 0.5 * np.spacing(np.abs(q).astype(np.float16)).astype(np.float64)
    return q, tol


def _assert_grad(grad, want, tol, f16):
    got = grad.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == (np.float16 if f16 else np.float32)
    if tol is None:
        assert _same_f16(got, want) if f16 else got.tobytes() == want.tobytes()
    else:
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= tol).all(), f"{int((err > tol).sum())} elements beyond the allowance, worst {float((err / np.maximum(tol, 1e-300)).max()):.3g}"
        assert np.array_equal(got == 0, want == 0)


def _ws_counters():
    import project_features_autograd as pfa
    import voxproj_host as vh
    return vh.counters(pfa._workspace(DEV), DEV)


def _forward_and_check(oracle_mod, feats, occ, c2w, intr, opts, origin, vs, n_rows, reduce):
    """pfa.project_features(feats, ...) and the oracle on the same maps: counts exact, out by sum_criteria (mean: out * count).
    Returns (out, oracle hits, oracle counts, the counters of the call)."""
    import project_features_autograd as pfa
    B, V, H, W, C = feats.shape
    out, count = pfa.project_features(feats, torch.from_numpy(occ).to(DEV), torch.from_numpy(c2w).reshape(-1).to(DEV),
                                      torch.from_numpy(intr).to(DEV), opts, origin, vs, n_rows, reduce=reduce)
    ctr = _ws_counters()
    f_np = feats.detach().float().cpu().numpy()
    ref_c, ref_o = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32)
    r = oracle_mod.project_features(f_np, occ, c2w.reshape(-1), intr, opts, origin, vs, ref_c, ref_o, want_f64=True)
    assert r["rc"] == 0
    assert np.array_equal(count.cpu().numpy(), ref_c)
    assert ctr["bad_id"] == 0
    got = out.detach().double() * count.clamp(min=1)[:, None].double() if reduce == "mean" else out.detach()
    split = ref_c > ctr["part_t"] if ctr["n_split"] > 0 else None
    assert_sums_vs_oracle(got, r, f_np, ref_c, split=split, oracle32=ref_o, dev=str(DEV))
    return out, r["hits"], ref_c, ctr


def _grad_case(oracle_mod, feats, occ, c2w, intr, opts, origin, vs, n_rows, reduce, seed, leaf=None, to_leaf=None):
    """Forward, then autograd.grad of out with a random upstream gradient; the gradient of ``leaf`` (default ``feats``)
    against the oracle's.  ``to_leaf`` maps a [B,V,H,W,C] array to the leaf's layout."""
    leaf = feats if leaf is None else leaf
    out, hits, ref_c, ctr = _forward_and_check(oracle_mod, feats, occ, c2w, intr, opts, origin, vs, n_rows, reduce)
    g = torch.randn(n_rows, feats.shape[-1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    (grad,) = torch.autograd.grad(out, leaf, g)
    f16 = feats.dtype == torch.float16
    want, tol = _grad_ref(hits, ref_c, g.cpu().numpy(), reduce, f16)
    if to_leaf is not None:
        want, tol = to_leaf(want), (None if tol is None else to_leaf(tol))
    _assert_grad(grad, want, tol, f16)
    return ctr


def _room(V, W, H, n_vox, seed, room=(5.0, 4.0, 2.4)):
    s = make_scene(n_vox, V, W, H, seed=seed, room=room)
    return s, s.occ[None].astype(np.int64), np.ascontiguousarray(s.c2w[:V]), s.intr[None].astype(np.float32)


def _feats(B, V, H, W, C, dtype, seed):
    f = make_features_np(B * V, H, W, C, seed=seed).reshape(B, V, H, W, C)
    return torch.from_numpy(f).to(DEV).to(dtype).requires_grad_(True)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("C,dtype", [(512, torch.float16), (67, torch.float32), (64, torch.float32), (1024, torch.float32)])
def test_autograd_multi_view_against_the_oracle(oracle_mod, C, dtype, reduce):
    """Six views, default heavy threshold (min(256 + 64*B*V, 2048) = 640): the large voxels of the close views are split into
    parts.  Backward: fp16 C = 512 -> k_render_walk<8,1,_Float16> (voxproj.hip:568), the LSeg production case; fp32 C = 67 ->
    the scalar forward (vec_ok == 0, project_gather) and <1,4,float> (:574); C = 64, 1024 -> <4,2,float> (:573)."""
    s, occ, c2w, intr = _room(6, 96, 72, 1000, seed=61, room=(3.0, 2.5, 2.0))     # 12 voxels above 640 pixels
    feats = _feats(1, 6, 72, 96, C, dtype, seed=C)
    ctr = _grad_case(oracle_mod, feats, occ, c2w, intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1, reduce, seed=C)
    assert ctr["n_split"] > 0, ctr


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_autograd_one_view_close_up_with_parts(oracle_mod, workspace_option, reduce):
    """B*V = 1 on the first frame of a hand-held trajectory (a close-up dwell): the one-view plan, its large voxels cut into parts
    (VP_OPT_ONE_VIEW_SPLIT = 16, VP_OPT_PART_PIXELS = 8) and added by k_combine_parts; backward <8,1,_Float16> at C = 64."""
    import voxproj_host as vh
    workspace_option(vh.VP_OPT_ONE_VIEW_SPLIT, 16)
    workspace_option(vh.VP_OPT_PART_PIXELS, 8)
    s = make_scene(6000, 40, 80, 60, seed=4, trajectory=True)
    feats = _feats(1, 1, 60, 80, 64, torch.float16, seed=5)
    ctr = _grad_case(oracle_mod, feats, s.occ[None].astype(np.int64), np.ascontiguousarray(s.c2w[:1]), s.intr[None], s.opts(),
                     s.grid_origin, s.voxel_size, s.n_vox + 1, reduce, seed=6)
    assert ctr["n_split"] > 0 and ctr["n_parts"] > ctr["n_split"], ctr


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_autograd_two_batches_with_different_grids(oracle_mod, reduce):
    """B = 2: batch 1's grid is batch 0's with a third of its voxels removed and the IDs of the rest permuted; batch 1 sees the
    views rolled by one.  fp32 C = 64."""
    s, occ, c2w, intr = _room(4, 96, 64, 2000, seed=71)
    rng = np.random.default_rng(71)
    o1 = occ[0].copy()
    nz = np.flatnonzero(o1)
    o1.reshape(-1)[nz] = rng.permutation(o1.reshape(-1)[nz])
    o1.reshape(-1)[rng.choice(nz, nz.size // 3, replace=False)] = 0
    occ2 = np.stack([occ[0], o1])
    c2w2 = np.stack([c2w, np.roll(c2w, 1, axis=0)])
    feats = _feats(2, 4, 64, 96, 64, torch.float32, seed=72)
    _grad_case(oracle_mod, feats, occ2, c2w2, np.repeat(intr, 2, axis=0), s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1,
               reduce, seed=73)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_autograd_through_a_permuted_lseg_layout(oracle_mod, reduce):
    """feats = the [B,V,H,W,C] permute of an LSeg-layout [B,V,C,H,W] float16 leaf (not contiguous): the gradient has the leaf's
    shape and is the oracle gradient in the leaf's layout."""
    s, occ, c2w, intr = _room(3, 64, 48, 2000, seed=81)
    lseg = torch.from_numpy(make_features_np(3, 48, 64, 64, seed=81)).permute(0, 3, 1, 2)[None].contiguous().to(DEV).half()
    lseg.requires_grad_(True)
    feats = lseg.permute(0, 1, 3, 4, 2)
    assert not feats.is_contiguous()
    _grad_case(oracle_mod, feats, occ, c2w, intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1, reduce, seed=82, leaf=lseg,
               to_leaf=lambda a: np.ascontiguousarray(a.transpose(0, 1, 4, 2, 3)))


def test_autograd_expanded_and_strided_upstream_gradients(oracle_mod):
    """out.sum() hands backward an expanded gradient (stride 0); a column slice of a wider tensor a strided one."""
    s, occ, c2w, intr = _room(3, 64, 48, 2000, seed=91)
    n_rows, C = s.n_vox + 1, 64
    for reduce in ("sum", "mean"):
        feats = _feats(1, 3, 48, 64, C, torch.float32, seed=92)
        out, hits, ref_c, _ = _forward_and_check(oracle_mod, feats, occ, c2w, intr, s.opts(), s.grid_origin, s.voxel_size, n_rows,
                                                 reduce)
        out.sum().backward(retain_graph=True)
        want, tol = _grad_ref(hits, ref_c, np.ones((n_rows, C), np.float32), reduce, False)
        _assert_grad(feats.grad, want, tol, False)
        wide = torch.randn(n_rows, 3 * C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(93))
        g = wide[:, ::3]
        assert g.stride() == (3 * C, 3)
        (grad,) = torch.autograd.grad(out, feats, g)
        want, tol = _grad_ref(hits, ref_c, g.contiguous().cpu().numpy(), reduce, False)
        _assert_grad(grad, want, tol, False)


def test_autograd_backward_after_later_forwards_on_other_scenes(oracle_mod):
    """Two forwards on different scenes through the module's one shared workspace, then backward of the first, then of the
    second: each gradient equals its own oracle gradient (the forward keeps its hit image, not the workspace's)."""
    cases = []
    for k, (W, H, C, dtype) in enumerate([(64, 48, 64, torch.float16), (96, 64, 67, torch.float32)]):
        s, occ, c2w, intr = _room(3 + k, W, H, 1500 + 700 * k, seed=101 + k)
        feats = _feats(1, 3 + k, H, W, C, dtype, seed=111 + k)
        out, hits, ref_c, _ = _forward_and_check(oracle_mod, feats, occ, c2w, intr, s.opts(), s.grid_origin, s.voxel_size,
                                                 s.n_vox + 1, "mean" if k else "sum")
        cases.append((feats, out, hits, ref_c, "mean" if k else "sum"))
    for k, (feats, out, hits, ref_c, reduce) in enumerate(cases):
        g = torch.randn(out.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(121 + k))
        out.backward(g)
        f16 = feats.dtype == torch.float16
        want, tol = _grad_ref(hits, ref_c, g.cpu().numpy(), reduce, f16)
        _assert_grad(feats.grad, want, tol, f16)


def test_autograd_on_a_side_stream(oracle_mod):
    """Forward and backward under a non-default torch.cuda.Stream."""
    s, occ, c2w, intr = _room(4, 96, 64, 2000, seed=131)
    side = torch.cuda.Stream(DEV)
    feats = _feats(1, 4, 64, 96, 512, torch.float16, seed=132)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _grad_case(oracle_mod, feats, occ, c2w, intr, s.opts(), s.grid_origin, s.voxel_size, s.n_vox + 1, "sum", seed=133)
    side.synchronize()
