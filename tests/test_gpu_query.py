"""GPU tests of the text query (vp_query_features through voxproj_host.query_features) against the float64 formula of
query_reference.py: every dispatch path (fp16 / fp32 rows, 16-byte or element loads, one or several channel chunks, partial
P-tiles and row tiles), optional outputs, zero / non-finite / tied rows, the scale range, 64-bit offsets, determinism and
row independence; query_voxel_features.py end to end on a synthetic aggregation."""
import os

import numpy as np
import pytest
import torch

import query_reference as qr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rows(N, C, dtype, seed, misalign=False, extra=0):
    """[N, C] rows on the GPU; misalign: the first row starts one element past a 16-byte boundary; extra: row stride C + extra."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    stride = C + extra
    flat = torch.randn(N * stride + 1, generator=g).to(dtype).to(DEV)
    base = flat[1:] if misalign else flat[:-1]
    return base.as_strided((N, C), (stride, 1))


def _text(P, C, seed, misalign=False):
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    t = torch.randn(P * C + 1, generator=g).to(DEV)
    return (t[1:] if misalign else t[:-1]).view(P, C)


def _run(rows, text, scale=1.0, **kw):
    import voxproj_host as vh
    lab, lg, mg = vh.query_features(rows, text, scale, **kw)
    torch.cuda.synchronize()
    return lab, lg, mg


# (dtype, N, C, P, misaligned rows/text, extra row stride): every kernel variant (fp16/fp32 x vector/element loads), one and
# several channel chunks (fp16 > 512, fp32 > 256 channels), C below one slot, P-tiles full / partial / many, row tails
CASES = [
    (torch.float16, 1, 1, 1, False, 0),
    (torch.float16, 15, 7, 2, False, 0),
    (torch.float16, 16, 8, 13, False, 0),
    (torch.float16, 17, 31, 15, False, 3),
    (torch.float16, 1000, 32, 16, True, 0),
    (torch.float16, 1000, 64, 17, False, 8),
    (torch.float16, 100003, 512, 13, False, 0),
    (torch.float16, 1000, 100, 64, True, 0),
    (torch.float16, 17, 768, 100, False, 0),
    (torch.float16, 1000, 512, 1024, False, 0),
    (torch.float16, 1000, 2048, 100, True, 5),
    (torch.float16, 16, 2048, 1024, False, 0),
    (torch.float32, 1, 1, 1, False, 0),
    (torch.float32, 15, 7, 2, True, 0),
    (torch.float32, 16, 8, 13, False, 0),
    (torch.float32, 17, 31, 15, False, 1),
    (torch.float32, 1000, 32, 16, False, 0),
    (torch.float32, 1000, 64, 17, True, 0),
    (torch.float32, 100003, 512, 13, False, 4),
    (torch.float32, 1000, 100, 64, False, 0),
    (torch.float32, 17, 768, 100, True, 0),
    (torch.float32, 1000, 512, 1024, False, 0),
    (torch.float32, 1000, 2048, 15, False, 0),
]


@pytest.mark.parametrize("dtype,N,C,P,mis,extra", CASES,
                         ids=[f"{'f16' if c[0] == torch.float16 else 'f32'}-N{c[1]}-C{c[2]}-P{c[3]}{'-mis' if c[4] else ''}"
                              f"{'-s' + str(c[5]) if c[5] else ''}" for c in CASES])
def test_query_paths_against_float64(dtype, N, C, P, mis, extra):
    rows = _rows(N, C, dtype, seed=N + C + P, misalign=mis, extra=extra)
    text = _text(P, C, seed=C * 7 + P, misalign=mis)
    lab, lg, mg = _run(rows, text)
    r = rows.float().cpu().numpy()
    t = text.cpu().numpy()
    qr.check(r, t, 1.0, lab.cpu().numpy(), lg.cpu().numpy(), mg.cpu().numpy())
    assert lab.dtype == torch.int32 and lg.shape == (N, P) and mg.shape == (N,)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_optional_outputs_do_not_change_labels(dtype):
    import voxproj_host as vh
    rows = _rows(5000, 512, dtype, seed=3)
    text = _text(100, 512, seed=3)
    rows[7] = float("nan")
    full = _run(rows, text, check=False)
    lab0 = full[0].cpu()
    for want_logits in (False, True):
        for want_margin in (False, True):
            lab, lg, mg = vh.query_features(rows, text, want_logits=want_logits, want_margin=want_margin, check=False)
            assert (lg is not None) == want_logits and (mg is not None) == want_margin
            assert torch.equal(lab.cpu(), lab0)
            if lg is not None:
                assert lg.cpu().numpy().tobytes() == full[1].cpu().numpy().tobytes()
            if mg is not None:
                assert mg.cpu().numpy().tobytes() == full[2].cpu().numpy().tobytes()
    # the counter: raised with check, counted exactly through the raw entry point
    with pytest.raises(vh.VoxprojError, match="1 row"):
        vh.query_features(rows, text)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    labels = torch.empty(5000, dtype=torch.int32, device=DEV)
    ws = torch.empty(vh.lib().vp_query_workspace_bytes(100, 512) + 256, dtype=torch.uint8, device=DEV)
    vh.check(vh.lib().vp_query_features(rows.data_ptr(), int(dtype == torch.float16), 5000, 512, 512, text.contiguous().data_ptr(),
                                        100, 1.0, None, labels.data_ptr(), None, cnt.data_ptr(), (ws.data_ptr() + 255) & ~255,
                                        ws.numel() - 256, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(cnt.item()) == 1 and torch.equal(labels.cpu(), lab0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("scale", [1.0, 1 / 0.07])
def test_special_rows(dtype, scale):
    N, C, P = 70, 64, 13
    rows = _rows(N, C, dtype, seed=11).contiguous()
    rows[0] = 0.0                               # zero row: logits 0, label 0, margin 0
    rows[1, 5] = float("inf")                   # non-finite rows: label -1, NaN
    rows[2, 63] = float("nan")
    rows[3, 0] = float("-inf")
    text = _text(P, C, seed=11).clone()
    text[9] = text[4]                           # an exact duplicate (and a scaled one): ties go to the lowest index
    text[12] = text[4] * 3.0
    rows[10] = text[4].to(dtype)                # rows pointing at the duplicated prompt
    rows[11] = (text[4] * 0.25).to(dtype)
    lab, lg, mg = _run(rows, text, scale, check=False)
    lab, lg, mg = lab.cpu().numpy(), lg.cpu().numpy(), mg.cpu().numpy()
    assert lab[0] == 0 and (lg[0] == 0).all() and mg[0] == 0
    assert (lab[1:4] == -1).all() and np.isnan(lg[1:4]).all() and np.isnan(mg[1:4]).all()
    assert lab[10] == 4 and lab[11] == 4
    qr.check(rows.float().cpu().numpy(), text.cpu().numpy(), scale, lab, lg, mg)
    # P = 1: margin 1, also for the zero row
    lab1, _, mg1 = _run(rows[4:], text[:1], scale, check=False)
    assert (lab1.cpu() == 0).all() and (mg1.cpu() == 1).all()
    _, _, mz = _run(rows[:1], text[:1], scale)
    assert float(mz) == 1.0


def test_scale_range_gives_the_unscaled_labels():
    N, C, P = 4000, 512, 100
    base = _rows(N, C, torch.float32, seed=21).contiguous()
    text = _text(P, C, seed=21)
    lab0, lg0, _ = _run(base, text)
    for f in (1e-15, 1e15):
        rows = base * f
        lab, lg, mg = _run(rows, text)
        qr.check(rows.double().cpu().numpy(), text.cpu().numpy(), 1.0, lab.cpu().numpy(), lg.cpu().numpy(), mg.cpu().numpy())
        L64, lab64, _, _ = qr.query64(base.cpu().numpy(), text.cpu().numpy())
        srt = np.sort(L64, axis=1)
        clear = srt[:, -1] - srt[:, -2] > 2 * qr.bound(C)
        assert np.array_equal(lab.cpu().numpy()[clear], lab0.cpu().numpy()[clear])
    # fp16 rows in the subnormal range (|x| < 2^-14), including rows made only of subnormals
    h = (base[:, :] * 2.0 ** -20).half()
    assert (h.abs() < 2.0 ** -14).float().mean() > 0.99 and (h != 0).float().mean() > 0.9
    lab, lg, mg = _run(h, text)
    qr.check(h.double().cpu().numpy(), text.cpu().numpy(), 1.0, lab.cpu().numpy(), lg.cpu().numpy(), mg.cpu().numpy())
    # and a row holding one normal element among subnormals keeps the subnormals' contribution
    h2 = (base[:8] * 2.0 ** -22).half()
    h2[:, 0] = 2.0 ** -13
    lab, lg, mg = _run(h2, text)
    qr.check(h2.double().cpu().numpy(), text.cpu().numpy(), 1.0, lab.cpu().numpy(), lg.cpu().numpy(), mg.cpu().numpy())


def test_run_to_run_slices_and_side_stream():
    N, C, P = 50_000, 512, 100
    for dtype in (torch.float16, torch.float32):
        rows = _rows(N, C, dtype, seed=31)
        text = _text(P, C, seed=31)
        a = [x.cpu().numpy() for x in _run(rows, text)]
        b = [x.cpu().numpy() for x in _run(rows, text)]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        for lo, hi in ((0, 1), (5, 21), (17, 4113), (49_990, 50_000)):
            s = [x.cpu().numpy() for x in _run(rows[lo:hi], text)]
            assert all(x.tobytes() == y[lo:hi].tobytes() for x, y in zip(s, a)), (lo, hi)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            import voxproj_host as vh
            out = vh.query_features(rows, text, check=False)
        side.synchronize()
        assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(out, a))


def test_beyond_2_31_elements():
    import voxproj_host as vh
    C, P = 512, 13
    N = (1 << 31) // C + 4099                    # N * C > 2^31 fp16 elements (~4.3 GB)
    rows = torch.empty((N, C), dtype=torch.float16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(41)
    for lo in range(0, N, 1 << 20):
        rows[lo:lo + (1 << 20)].normal_(generator=g)
    text = _text(P, C, seed=41)
    lab, _, mg = vh.query_features(rows, text, want_logits=False)
    tail = rows[N - 5000:]
    lab_t, lg_t, mg_t = _run(tail, text)
    assert torch.equal(lab[N - 5000:], lab_t) and torch.equal(mg[N - 5000:], mg_t)
    qr.check(tail.float().cpu().numpy(), text.cpu().numpy(), 1.0, lab_t.cpu().numpy(), lg_t.cpu().numpy(), mg_t.cpu().numpy())
    head = rows[:3000]
    lab_h, _, _ = _run(head, text)
    assert torch.equal(lab[:3000], lab_h)
    del rows
    torch.cuda.empty_cache()


def _composite(feats, text, scale=1.0):
    """The obvious torch version: F.normalize, matmul, argmax (float32)."""
    import torch.nn.functional as F
    lg = scale * (F.normalize(feats.float(), dim=1) @ F.normalize(text.float(), dim=1).T)
    return lg, lg.argmax(dim=1)


def _clear(lg64, C, scale=1.0):
    s = np.sort(lg64, axis=1)
    return s[:, -1] - s[:, -2] > 2 * qr.bound(C, scale)


def test_query_script_end_to_end(tmp_path):
    import aggregate_voxel_features_onthefly as agg
    import build_sparse_occupancy as bso
    import prepare_tensor_data as ptd
    import query_voxel_features as qvf
    import voxproj_host as vh
    from test_gpu_render import _write_files
    s, ply, lseg, cam_json = _write_files(tmp_path)
    agg.main(["--mode", "fast", "--lseg_dir", str(lseg), "--cam_params", str(cam_json), "--voxel_ply", str(ply),
              "--checkpoint_dir", str(tmp_path / "agg")])
    pt = tmp_path / "agg" / f"ALL_nonzero_voxel_features_4_vox{s.n_vox}.pt"
    d = torch.load(pt)
    feats, xyz = d["avg_feats"], d["xyz"].float()
    C = feats.shape[1]
    prompts = ["wall", "floor", "chair", "table", "lamp"]
    text = np.random.default_rng(5).standard_normal((len(prompts), C)).astype(np.float32)
    np.save(tmp_path / "text.npy", text)
    scale = 1 / 0.07
    common = ["--text_emb", str(tmp_path / "text.npy"), "--prompt", *prompts, "--logit_scale", str(scale)]
    lg_t, lab_t = _composite(feats.to(DEV), torch.from_numpy(text).to(DEV), scale)
    L64, _, _, _ = qr.query64(feats.float().numpy(), text, scale)
    clear = _clear(L64, C, scale)
    assert clear.mean() > 0.9

    # voxels
    qvf.main(["voxels", *common, "--vox", str(pt), "--out", str(tmp_path / "v.npz")])
    z = np.load(tmp_path / "v.npz")
    assert z["labels"].dtype == np.int16 and z["logits"].dtype == np.float32 and z["colors"].dtype == np.uint8
    assert z["logits"].shape == (len(feats), len(prompts)) and list(z["prompts"]) == prompts
    assert np.array_equal(z["labels"][clear], lab_t.cpu().numpy()[clear])
    assert np.abs(z["logits"] - lg_t.cpu().numpy()).max() <= 2 * qr.bound(C, scale)
    assert np.array_equal(z["colors"], qr.palette(len(prompts))[z["labels"]])
    head = open(tmp_path / "v_colored_voxels.ply").read().split("end_header\n")
    assert f"element vertex {len(feats)}" in head[0] and len(head[1].splitlines()) == len(feats)

    # gaussians: centres jittered around a subset of voxels, map computed and given
    rng = np.random.default_rng(6)
    pick = rng.integers(0, len(xyz), 3000)
    mu = (xyz.numpy()[pick] + rng.uniform(-0.2, 0.2, (3000, 3)) * s.voxel_size).astype(np.float32)
    np.save(tmp_path / "mu.npy", mu)
    qvf.main(["gaussians", *common, "--vox", str(pt), "--gauss", str(tmp_path / "mu.npy"), "--out", str(tmp_path / "g.npz")])
    import voxel_to_gaussian_map
    g2v = voxel_to_gaussian_map.map_gaussians_to_voxels(xyz, torch.from_numpy(mu)).numpy()
    zg = np.load(tmp_path / "g.npz")
    assert zg["labels"].dtype == np.int16 and zg["logits"].shape == (3000, len(prompts))
    assert np.array_equal(zg["labels"], z["labels"][g2v]) and np.array_equal(zg["logits"], z["logits"][g2v])
    assert np.array_equal(zg["labels"][clear[g2v]], lab_t.cpu().numpy()[g2v][clear[g2v]])
    np.save(tmp_path / "g2v.npy", g2v)
    qvf.main(["gaussians", *common, "--vox", str(pt), "--gauss", str(tmp_path / "mu.npy"), "--map", str(tmp_path / "g2v.npy"),
              "--out", str(tmp_path / "g2.npz")])
    assert np.load(tmp_path / "g2.npz")["labels"].tobytes() == zg["labels"].tobytes()
    assert os.path.exists(tmp_path / "g_colored_gaussians.ply")

    # views: labels are the voxel labels of the first-hit voxel; the saved logits give the saved confidence
    out_dir = tmp_path / "views"
    qvf.main(["views", *common, "--features_pt", str(pt), "--voxel_ply", str(ply), "--cam_params", str(cam_json),
              "--views", "IMG0001", "IMG0003", "--out_dir", str(out_dir), "--save_logits"])
    vs, origin, _, _ = bso.extract_voxel_params(str(ply))
    occ3 = bso.build_occupancy(bso.read_voxel_ply(str(ply)), origin, vs, device=DEV)
    n_rows = int(occ3.max()) + 1
    zyx = d["voxel_coords"].long().to(DEV)
    row_lab = np.full(n_rows, -1, np.int64)
    row_lab[occ3[zyx[:, 0], zyx[:, 1], zyx[:, 2]].long().cpu().numpy()] = z["labels"]
    by_name, cams = ptd.load_camera_params(str(cam_json))
    for name in ("IMG0001", "IMG0003"):
        intr, c2w = ptd.camera_for(by_name[name], cams, 0.5)
        ids = vh.first_hit_ids(occ3[None].long().contiguous(), c2w.reshape(-1).to(DEV), intr.reshape(1, 4).to(DEV),
                               agg.ray_opts(48, 32, vs), origin, vs, 32, 48, n_rows)[0, 0].cpu().numpy()
        lab = np.load(out_dir / f"{name}_labels.npy")
        conf = np.load(out_dir / f"{name}_confidence.npy")
        lg = np.load(out_dir / f"{name}_logits.npy")
        assert lab.dtype == np.int16 and lab.shape == (32, 48) and conf.dtype == np.float32 and lg.dtype == np.float16
        assert lg.shape == (len(prompts), 32, 48)
        assert np.array_equal(lab, row_lab[ids]) and (lab >= 0).mean() > 0.3
        assert (conf[lab < 0] == 0).all()
        # logit_confidence_map.py's formula in NumPy on the saved fp16 logits
        x = lg.astype(np.float64)
        e = np.exp(x - x.max(axis=0, keepdims=True))
        p = np.sort(e / e.sum(axis=0, keepdims=True), axis=0)
        conf_np = p[-1] - p[-2]
        m = lab >= 0
        assert np.abs(conf_np[m] - conf[m]).max() <= 2e-3 * scale
