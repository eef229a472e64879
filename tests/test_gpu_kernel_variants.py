"""Every kernel instantiation the host-side dispatchers of csrc/voxproj.hip can select, run at the widths where it differs from
its neighbours -- not only the ones the production shapes reach.  Each case names the instantiation and the host rule that picks
it (file:line in csrc/voxproj.hip unless another file is named).

  A  the scalar fp32 projector path (K = 4, VEC = 1: a pass of 256 channels as ch = k*64 + lane), which vec_ok == 0 selects
     (project_gather, vp_project.h): C % 4 != 0, or feats / out not 16-byte aligned.  Against the oracle: hit image and counts exact, sums
     bit-exact when serial, tests/sum_criteria.py when split; misaligned rows give the aligned run's bytes.
  B  k_aggregate_view_f16 (vp_aggregate.h) at every width class, against oracle.aggregate_views bit for bit.
  C  k_upsample_hwc<TS, TD, VEC, NV> for every register-window size (VP_UPS, voxproj.hip:793-800) and both transposes, against
     oracle/resize_oracle.py bit for bit and a float64 bilinear evaluation within one fp16 ulp.
"""
import numpy as np
import pytest
import torch

from sum_criteria import assert_sums, assert_sums_vs_oracle
from synthetic_scene import make_features_np, make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SERIAL = 10 ** 8                  # a heavy threshold no voxel of these scenes reaches: every row summed by one wavefront
WIDE = [67, 255, 257, 513, 1001]  # C % 4 != 0, passes of 256 channels: one (partial), one, two, three, four (the last ragged)


def _offset_empty(shape, dtype, off, fill=0.0, guard=-7.0):
    """A contiguous tensor of ``shape`` whose first element lies ``off`` elements into its allocation (torch's allocator hands out
    blocks aligned far beyond 16 bytes, so off = 1 puts it 4 (fp32) or 2 (fp16) bytes off a 16-byte boundary), filled with
    ``fill``; the allocation around it holds ``guard``.  Returns (view, allocation)."""
    n = int(np.prod(shape))
    buf = torch.full((n + off + 8,), guard, dtype=dtype, device=DEV)
    view = buf[off:off + n].view(shape)
    view.fill_(fill)
    assert view.is_contiguous() and (off == 0 or view.data_ptr() % 16 != 0)
    return view, buf


def _guards_intact(view, buf, guard=-7.0):
    off = view.storage_offset()
    n = view.numel()
    return bool((buf[:off] == guard).all()) and bool((buf[off + n:] == guard).all())


def _scene(V, C, seed, W=48, H=32):
    s = make_scene(2000, V, W, H, seed=seed, room=(5.0, 4.0, 2.4))
    return s, make_features_np(V, H, W, C, seed=seed)[None]


def _tensors(s, feats, dev, views=None):
    views = range(feats.shape[1]) if views is None else views
    return dict(feats=torch.from_numpy(np.ascontiguousarray(feats[:, views])).to(dev),
                occ=torch.from_numpy(s.occ[None].astype(np.int64)).to(dev),
                vmi=torch.from_numpy(np.ascontiguousarray(s.c2w[views])).reshape(-1).contiguous().to(dev),
                intr=torch.from_numpy(s.intr[None]).to(dev), opts=[float(x) for x in s.opts()],
                origin=[float(x) for x in s.grid_origin])


def _call(t, s, ws, count, out, **kw):
    import voxproj_host
    return voxproj_host.project_features_raw(t["feats"], t["occ"], t["vmi"], t["intr"], t["opts"], count, out, t["origin"],
                                             s.voxel_size, workspace=ws, **kw)


def _oracle(oracle_mod, s, feats, want_f64=True):
    n_rows, C = s.n_vox + 1, feats.shape[-1]
    count, out = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32)
    r = oracle_mod.project_features(feats, s.occ[None].astype(np.int64), s.c2w[:feats.shape[1]].reshape(-1), s.intr[None], s.opts(),
                                    s.grid_origin, s.voxel_size, count, out, want_f64=want_f64)
    assert r["rc"] == 0
    return r, count, out


def _oracle_one_view_calls(oracle_mod, s, feats):
    """One oracle call per view accumulating into the same outputs (K.cu:77,88: +=), the float64 sums of the same pixels and of
    their |addend| (tests/sum_criteria.py), and every view's own pixel counts."""
    n_rows, V, C = s.n_vox + 1, feats.shape[1], feats.shape[-1]
    count, out, nviews = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32), np.zeros(n_rows, np.int32)
    ref64, abs64, per_view = np.zeros((n_rows, C)), np.zeros((n_rows, C)), []
    for v in range(V):
        c1 = np.zeros(n_rows, np.int32)
        f = np.ascontiguousarray(feats[:, v:v + 1])
        r = oracle_mod.project_features(f, s.occ[None].astype(np.int64), s.c2w[v].reshape(-1), s.intr[None], s.opts(), s.grid_origin,
                                        s.voxel_size, c1, out, want_f64=True)
        ref64 += r["out64"]
        np.add.at(abs64, r["hits"][0, 0].reshape(-1), np.abs(f[0, 0].reshape(-1, C)).astype(np.float64))
        abs64[0] = 0
        count += c1
        nviews += c1 > 0
        per_view.append(c1)
    return count, out, nviews, ref64, abs64, per_view


# ------------------------------------------------------------------------------------------------------------------------------
# A. The scalar projector path at real widths
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDE)
@pytest.mark.parametrize("V", [3, 9])
def test_scalar_rows_multi_view_calls(oracle_mod, V, C):
    """k_gather<4,1,4,1>: project_with_rows' last arm (vp_project.h), taken when vec_ok == 0 (project_gather, C % 4 != 0).
    V = 9 on this small image is the small-image branch (project_gather_views, G32 = 4), V = 3 the other (G32 = 1): the scalar arm
    pins G = 1 in both.  Serial sums: the oracle's bits.  Heavy threshold 6: the voxels above part_t are summed in parts by the
    same kernel and added by k_combine_parts<4,1,4> (the same arm, project_combine)."""
    import voxproj_host
    dev = torch.device(DEV)
    s, feats = _scene(V, C, seed=500 + V + C)
    n_rows = s.n_vox + 1
    r, ref_c, ref_o = _oracle(oracle_mod, s, feats)
    t = _tensors(s, feats, dev)
    for heavy in (SERIAL, 6):
        ws = voxproj_host.Workspace()
        ws.set_option(voxproj_host.VP_OPT_HEAVY_THRESHOLD, heavy)
        count, out = torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, C, device=dev)
        _call(t, s, ws, count, out, sync=True)
        assert np.array_equal(voxproj_host.hit_image(ws, dev).cpu().numpy(), r["hits"])
        ctr = voxproj_host.counters(ws, dev)
        assert ctr["bad_id"] == 0 and ctr["box_miss"] == 0
        got_c, got_o = count.cpu().numpy(), out.cpu().numpy()
        assert np.array_equal(got_c, ref_c)
        if heavy == SERIAL:
            assert ctr["n_split"] == 0
            assert got_o.tobytes() == ref_o.tobytes()
        else:
            split = ref_c > ctr["part_t"]
            assert ctr["part_t"] == 6 and ctr["n_split"] == int(split.sum()) > 20
            assert got_o[~split].tobytes() == ref_o[~split].tobytes()          # one-wavefront rows keep the serial bits
            assert_sums_vs_oracle(got_o, r, feats, ref_c, split=split, oracle32=ref_o, dev=DEV)
        ws.release()
    assert (r["hits"] > 0).mean() > 0.9


@pytest.mark.parametrize("C", WIDE)
def test_scalar_rows_one_view_calls(oracle_mod, C):
    """Three one-view calls accumulating into the same outputs, in each of the three roles a one-view call can give a voxel:
    - serial: k_gather_one<4,1,4> (project_with_rows' last arm in project_gather_one, vp_project.h; one_view: plan_split, vp_plan.h), the oracle's bits;
    - split: VP_OPT_ONE_VIEW_SPLIT = 12, VP_OPT_PART_PIXELS = 5 (one_split, plan_split): parts summed by
      k_gather_one<4,1,4>, added by k_combine_parts<4,1,4> (project_combine);
    - workgroup: the A/B arm VP_OPT_ONE_VIEW_SPLIT = 0 with heavy threshold 6 (plan_split; heavy_blocks in project_gather_one): the voxels the march
      enlists are summed by a workgroup of k_gather_one (gather_voxel_block<4,1,4,GW_MERGED>, vp_gather.h).
    Counts and views-hit exact in all three; rows no voxel role split keep the oracle's bits; the others by sum_criteria."""
    import voxproj_host
    dev = torch.device(DEV)
    V = 3
    s, feats = _scene(V, C, seed=600 + C)
    n_rows = s.n_vox + 1
    ref_c, ref_o, ref_v, ref64, abs64, per_view = _oracle_one_view_calls(oracle_mod, s, feats)
    arms = {"serial": {voxproj_host.VP_OPT_HEAVY_THRESHOLD: SERIAL},
            "split": {voxproj_host.VP_OPT_ONE_VIEW_SPLIT: 12, voxproj_host.VP_OPT_PART_PIXELS: 5},
            "workgroup": {voxproj_host.VP_OPT_HEAVY_THRESHOLD: 6, voxproj_host.VP_OPT_ONE_VIEW_SPLIT: 0}}
    for arm, options in arms.items():
        ws = voxproj_host.Workspace()
        for opt, val in options.items():
            ws.set_option(opt, val)
        count, out = torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, C, device=dev)
        views = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        light = np.ones(n_rows, bool)           # rows every view summed with one wavefront
        moved = 0
        for v in range(V):
            _call(_tensors(s, feats, dev, [v]), s, ws, count, out, sync=True, views_hit=views)
            ctr = voxproj_host.counters(ws, dev)
            assert ctr["bad_id"] == 0 and ctr["box_miss"] == 0
            c1 = per_view[v]
            if arm == "serial":
                assert ctr["n_split"] == 0 and ctr["n_heavy"] == 0
            elif arm == "split":
                big = c1[c1 > 12]
                assert (ctr["part_t"], ctr["part_px"]) == (12, 5)
                assert ctr["n_split"] == len(big) and ctr["n_parts"] == int(np.sum((big + 4) // 5))
                light &= c1 <= 12
                moved += len(big)
            else:
                assert ctr["n_split"] == 0 and ctr["n_heavy"] == int((c1 > 6).sum())
                light &= c1 <= 6
                moved += int((c1 > 6).sum())
        got_c, got_o, got_v = count.cpu().numpy(), out.cpu().numpy(), views.cpu().numpy()
        assert np.array_equal(got_c, ref_c) and np.array_equal(got_v, ref_v), arm
        assert got_o[light].tobytes() == ref_o[light].tobytes(), arm
        if arm != "serial":
            assert moved > 5, arm
            assert_sums(got_o, ref64, abs64, ref_c, split=~light, oracle32=ref_o, dev=DEV)
        ws.release()


def _drop_in(front):
    if front == "compiled":
        import project_features_cuda as m      # ModuleNotFoundError = not built: run __graft_entry__.build()
        assert m.__file__.endswith(".so")
        return m.project_features_cuda
    import project_features_front
    return project_features_front.project_features_cuda_py


@pytest.mark.parametrize("front", ["compiled", "python"])
@pytest.mark.parametrize("C", [64, 512, 1000])
@pytest.mark.parametrize("V", [1, 3])
def test_misaligned_rows_take_the_scalar_path_with_the_aligned_bits(oracle_mod, heavy_threshold, front, C, V):
    """C % 4 == 0, but ``feats`` or ``out`` is a contiguous view 4 bytes off a 16-byte boundary: the drop-in module accepts it
    (VP_CHECK_INPUT checks device and contiguity only, project_features_ext.cpp:25-27), and vec_ok == 0 (project_gather)
    sends the call to k_gather_one<4,1,4> (V = 1) or k_gather<4,1,4,1> (V = 3), and its parts to
    k_combine_parts<4,1,4> (:68).  The summation order -- (view, y, x) per wavefront, parts in slot order -- and the part plan
    (k_worklist: pixel counts and part_px, vp_gather.h) do not depend on the row width class, so both misaligned runs leave the
    aligned run's bytes, serial and split alike; no byte around the misaligned ``out`` is written."""
    import project_features_front
    import voxproj_host
    dev = torch.device(DEV)
    fn = _drop_in(front)
    s, feats = _scene(V, C, seed=700 + V + C)
    n_rows = s.n_vox + 1
    r, ref_c, ref_o = _oracle(oracle_mod, s, feats)
    feats_t = torch.from_numpy(feats).to(dev)
    feats_off, _ = _offset_empty(feats.shape, torch.float32, 1)
    feats_off.copy_(feats_t)
    occ_t = torch.from_numpy(s.occ[None].astype(np.int64)).to(dev)
    vmi_t = torch.from_numpy(s.c2w[:V]).reshape(-1).contiguous().to(dev)
    intr_t = torch.from_numpy(s.intr[None]).to(dev)
    for heavy in (SERIAL, 6):
        heavy_threshold(heavy)
        res = {}
        for arm in ("aligned", "feats", "out"):
            count = torch.zeros(n_rows, dtype=torch.int32, device=dev)
            if arm == "out":
                out, buf = _offset_empty((n_rows, C), torch.float32, 1)
            else:
                out, buf = torch.zeros(n_rows, C, device=dev), None
            fn(feats_off if arm == "feats" else feats_t, occ_t, vmi_t, intr_t, torch.from_numpy(s.opts()), count, out,
               torch.tensor([False]), torch.from_numpy(s.grid_origin), float(s.voxel_size))
            ws = project_features_front.last_workspace(dev, front=front)
            assert np.array_equal(voxproj_host.hit_image(ws, dev).cpu().numpy(), r["hits"]), arm
            ctr = voxproj_host.counters(ws, dev)
            assert ctr["bad_id"] == 0 and ctr["box_miss"] == 0, arm
            if buf is not None:
                assert _guards_intact(out, buf), "a write outside the misaligned output"
            res[arm] = (count.cpu().numpy(), out.cpu().numpy(), ctr)
        got_c, got_o, ctr = res["aligned"]
        assert np.array_equal(got_c, ref_c)
        for arm in ("feats", "out"):
            assert np.array_equal(res[arm][0], ref_c), arm
            assert res[arm][1].tobytes() == got_o.tobytes(), f"{arm} misaligned: not the aligned run's bytes"
        if heavy == SERIAL:
            assert got_o.tobytes() == ref_o.tobytes()
        else:
            split = ref_c > ctr["part_t"]
            assert ctr["n_split"] == int(split.sum()) > 10
            assert got_o[~split].tobytes() == ref_o[~split].tobytes()
            assert_sums_vs_oracle(got_o, r, feats, ref_c, split=split, oracle32=ref_o, dev=DEV)


def test_scalar_rows_in_job_mode_with_a_gather_only_range(oracle_mod):
    """C = 257 (k_gather<4,1,4,1>) in a pipelined sequence: a VP_FLAG_PIPELINE call on rows [0, h), the gather-only call for
    [h, n_rows) (VP_FLAG_GATHER_ONLY, project_check and project_relist: the previous call's march and plan), then a whole pipelined
    call, all accumulating into the same outputs: the oracle called twice, bit for bit."""
    import voxproj_host
    dev = torch.device(DEV)
    V, C = 9, 257
    s, feats = _scene(V, C, seed=801)
    n_rows = s.n_vox + 1
    count_r, out_r = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32)
    for _ in range(2):
        oracle_mod.project_features(feats, s.occ[None].astype(np.int64), s.c2w.reshape(-1), s.intr[None], s.opts(), s.grid_origin,
                                    s.voxel_size, count_r, out_r)
    t = _tensors(s, feats, dev)
    ws = voxproj_host.Workspace()
    ws.set_option(voxproj_host.VP_OPT_HEAVY_THRESHOLD, SERIAL)
    count, out = torch.zeros(n_rows, dtype=torch.int32, device=dev), torch.zeros(n_rows, C, device=dev)
    h = n_rows // 3
    ws.set_row_range(0, h)
    _call(t, s, ws, count, out, sync=False, pipeline=True)
    ws.set_row_range(h, n_rows)
    _call(t, s, ws, count, out, sync=False, pipeline=True, gather_only=True)
    ws.set_row_range()
    _call(t, s, ws, count, out, sync=False, pipeline=True)
    voxproj_host.workspace_status(ws, dev)
    torch.cuda.synchronize()
    assert voxproj_host.counters(ws, dev)["box_miss"] == 0
    assert np.array_equal(count.cpu().numpy(), count_r)
    assert out.cpu().numpy().tobytes() == out_r.tobytes()
    ws.release()


# ------------------------------------------------------------------------------------------------------------------------------
# B. k_aggregate_view_f16 at every width class
# ------------------------------------------------------------------------------------------------------------------------------
def _f16_bits(a):
    """The binary16 bit patterns of ``a``, every NaN as the one quiet NaN 0x7e00: NaN payloads and signs are not part of
    the reference's arithmetic (torch and numpy make them as their hardware does)."""
    b = np.ascontiguousarray(a, dtype=np.float16).view(np.uint16).copy()
    b[np.isnan(np.asarray(a, dtype=np.float16))] = 0x7E00
    return b


@pytest.mark.parametrize("n_rows", [2, 121, 126, 131, 136])          # (n_rows - 1) % 4 = 1, 0, 1, 2, 3: the last workgroup partial
@pytest.mark.parametrize("C", [1, 3, 40, 255, 256, 257, 260, 512, 1001])
def test_per_view_fp16_fold_at_every_width(oracle_mod, C, n_rows):
    """vp_aggregate_view_f16 (voxproj.hip:862-874) launches k_aggregate_view_f16 over ceil((n_rows - 1) / 4) workgroups of four
    voxel wavefronts; the kernel takes its scalar branch (c += 64) for C % 4 != 0 (1, 3, 255, 257, 1001) and its vector loop
    (c += 256) otherwise: once for 40 and 256, twice for 260 and 512.  Five views against the
    dict loop (oracle.aggregate_views) and a numpy restatement of the running fp16 rows, bit for bit:
      - view 1: a per-view sum of 1e6 in the LAST channel (scalar branch / channel >= 256 for C > 256): flagged (AGG:303-304);
      - view 3: a NaN in channel C // 2: flagged;
      - views 2 and 4: 40000 in channel 0 of one voxel -- each row is finite, only the running fp16 sum overflows: NOT flagged
        (AGG:303-304 checks the per-view row);
      - voxels first seen in a later view: first_view and views words as the dict's insertion order and view counts;
      - after every call view_sum / view_count are zero in every channel."""
    import voxproj_host
    rng = np.random.default_rng(C * 1000 + n_rows)
    V = 5
    occ = np.zeros((2, 4, (n_rows - 1) // 4 + 1), np.int32)
    idx = rng.choice(occ.size, n_rows - 1, replace=False)
    occ.reshape(-1)[idx] = np.arange(1, n_rows)
    ids = np.arange(1, n_rows)
    r1, r3, r24 = (rng.choice(ids, 3, replace=False) if len(ids) >= 3 else (ids[0],) * 3)
    dev = torch.device(DEV)
    view_sum = torch.zeros(n_rows, C, device=dev)
    view_cnt = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    run16 = torch.zeros(n_rows, C, dtype=torch.float16, device=dev)
    views = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    first = torch.full((n_rows,), 2 ** 30, dtype=torch.int32, device=dev)
    flags = torch.zeros(V, dtype=torch.int32, device=dev)
    per_view, cnts = [], []
    exp_run = np.zeros((n_rows, C), np.float16)
    for v in range(V):
        cnt = (rng.random(n_rows) < 0.4).astype(np.int32) * rng.integers(1, 50, n_rows).astype(np.int32)
        cnt[0] = 0
        if v == 0:
            cnt[ids[0]] = 0                                       # (n_rows = 2: the one voxel enters at view 1)
        sums = (rng.standard_normal((n_rows, C)) * 30).astype(np.float32)
        if v == 1:
            cnt[r1] = max(cnt[r1], 1)
            sums[r1, C - 1] = 1e6                                 # -> inf in binary16
        if v == 3:
            cnt[r3] = max(cnt[r3], 1)
            sums[r3, C // 2] = np.nan
        if v in (2, 4):
            cnt[r24] = max(cnt[r24], 1)
            sums[r24, 0] = 40000.0                                # finite in binary16; 80000 is not
        sums *= (cnt > 0)[:, None]
        cnts.append(cnt)
        per_view.append(oracle_mod.dpf_select_outputs(occ, cnt, sums))
        with np.errstate(over="ignore", invalid="ignore"):
            f = sums.astype(np.float16)
            seen = np.stack(cnts[:-1]).any(axis=0) if v else np.zeros(n_rows, bool)
            hit = cnt > 0
            exp_run[hit & ~seen] = f[hit & ~seen]                                                     # AGG:310 clone
            both = hit & seen
            exp_run[both] = (exp_run[both].astype(np.float32) + f[both].astype(np.float32)).astype(np.float16)   # AGG:312
        view_sum.copy_(torch.from_numpy(sums))
        view_cnt.copy_(torch.from_numpy(cnt))
        voxproj_host.aggregate_view_f16(view_sum, view_cnt, run16, views, first, v, flags, v)
        assert int(torch.count_nonzero(view_cnt)) == 0 and int(torch.count_nonzero(view_sum)) == 0, f"scratch not clean after view {v}"
    assert flags.cpu().tolist() == [0, 1, 0, 1, 0]
    hit_any = np.stack(cnts) > 0
    assert np.array_equal(views.cpu().numpy(), hit_any.sum(axis=0).astype(np.int32))
    exp_first = np.where(hit_any.any(axis=0), hit_any.argmax(axis=0), 2 ** 30).astype(np.int32)
    assert np.array_equal(first.cpu().numpy(), exp_first)
    if n_rows > 8:
        assert (exp_first[hit_any.any(axis=0)] > 0).any()                     # voxels that entered after view 0
    assert np.array_equal(_f16_bits(run16.cpu().numpy()), _f16_bits(exp_run))
    if len(ids) >= 3:
        assert np.isinf(exp_run[r24, 0]) and np.isinf(exp_run[r1, C - 1]) and np.isnan(exp_run[r3, C // 2])
    with np.errstate(over="ignore"):                                          # the dict's fp16 "+=" overflows on purpose
        exp = oracle_mod.aggregate_views(per_view, [0.0, 0.0, 0.0], 0.1)
    ids_hit = torch.nonzero(views > 0).reshape(-1)
    ids_hit = ids_hit[torch.argsort(first[ids_hit].long() * n_rows + ids_hit)]
    zyx = np.stack(np.unravel_index([int(np.nonzero(occ.reshape(-1) == i)[0][0]) for i in ids_hit.tolist()], occ.shape), 1)
    assert np.array_equal(zyx.astype(np.int32), exp["voxel_coords"])
    assert np.array_equal(views[ids_hit].cpu().numpy(), exp["hit_count"])
    with np.errstate(invalid="ignore"):
        avg = (run16[ids_hit].float() / views[ids_hit].float()[:, None]).to(torch.float16).cpu().numpy()
    assert np.array_equal(_f16_bits(avg), _f16_bits(exp["avg_feats"]))


def test_parity_aggregator_at_the_production_width(oracle_mod, heavy_threshold):
    """The parity aggregator end to end at C = 512 (two iterations of k_aggregate_view_f16's vector loop, k_gather_one<2,4,*>
    per view): voxel_coords, hit_count and avg_feats byte-equal to oracle.dpf_select_outputs + oracle.aggregate_views."""
    from aggregate_voxel_features_onthefly import VoxelFeatureAggregator
    heavy_threshold(None)
    V, C = 3, 512
    s = make_scene(2000, V, 48, 32, seed=901, room=(5.0, 4.0, 2.4))
    feats = make_features_np(V, 32, 48, C, seed=901) * np.float32(8.0)
    n_rows = s.n_vox + 1
    per_view = []
    for v in range(V):
        cnt, sums = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32)
        oracle_mod.project_features(feats[None, v:v + 1], s.occ[None].astype(np.int64), s.c2w[v].reshape(-1), s.intr[None], s.opts(),
                                    s.grid_origin, s.voxel_size, cnt, sums)
        per_view.append(oracle_mod.dpf_select_outputs(s.occ, cnt, sums))
    exp = oracle_mod.aggregate_views(per_view, s.grid_origin.astype(np.float64), s.voxel_size)
    assert len(exp["hit_count"]) > 500 and (exp["hit_count"] > 1).any()
    agg = VoxelFeatureAggregator(torch.from_numpy(s.occ), s.grid_origin.astype(np.float64), s.voxel_size, C, "parity", DEV)
    agg.add_views(torch.from_numpy(feats).to(DEV), torch.from_numpy(s.c2w), torch.from_numpy(s.intr))
    r = agg.result()
    assert np.array_equal(r["voxel_coords"].numpy(), exp["voxel_coords"]) and np.array_equal(r["hit_count"].numpy(), exp["hit_count"])
    assert r["avg_feats"].numpy().tobytes() == exp["avg_feats"].tobytes()


# ------------------------------------------------------------------------------------------------------------------------------
# C. The up-sampler's instantiation matrix
# ------------------------------------------------------------------------------------------------------------------------------
# (h, w) -> (H, W): integer and non-integer up-sampling, down-sampling, up in one axis and down in the other, h = 1 and w = 1
# (every output column of w = 1 takes the right-border tap alone: two == false).  h*w is not a multiple of 8 except for
# (4, 6), so the fp16 transpose is the element-wise k_chw_to_hwc<_Float16> (voxproj.hip:803-806) for every other size.
SIZES = [((5, 7), (10, 14)), ((5, 7), (12, 17)), ((9, 13), (5, 7)), ((7, 9), (4, 20)), ((1, 6), (3, 11)), ((6, 1), (11, 3)),
         ((4, 6), (9, 13))]


def _check_upsample(arr, H, W, keep, src_off=0, out_off=0):
    import voxproj_host
    from oracle import resize_oracle as ro
    C, h, w = arr.shape
    src = torch.from_numpy(arr).to(DEV)
    if src_off:
        s2, _ = _offset_empty(arr.shape, src.dtype, src_off)
        s2.copy_(src)
        src = s2
    dst_dtype = torch.float16 if keep else torch.float32
    out, buf = _offset_empty((H, W, C), dst_dtype, out_off, fill=float("nan"))
    got = voxproj_host.upsample_features(src, H, W, keep_dtype=keep, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _guards_intact(out, buf), "a write outside the destination"
    got = got.cpu().numpy()
    exp = ro.upsample_features(arr, H, W, keep_dtype=keep)
    assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), f"C={C} {h}x{w} -> {H}x{W} keep={keep}"
    if H >= h and W >= w:
        # float64 bilinear with half-pixel centres: the results agree within one fp16 ulp of the value
        r16 = np.transpose(ro.bilinear_f64(arr, H, W), (1, 2, 0)).astype(np.float16)
        ulp = np.spacing(np.abs(r16)).astype(np.float64)
        scale = np.abs(arr.astype(np.float64)).max()
        assert (np.abs(got.astype(np.float64) - r16.astype(np.float64)) <= ulp + 4e-6 * scale).all()


def _maps(C, dt, seed):
    rng = np.random.default_rng(seed)
    for (h, w), (H, W) in SIZES:
        arr = rng.standard_normal((C, h, w)).astype(dt)
        arr.reshape(-1)[::11] *= 40                                        # some large values (fp16 rounding at coarse ulps)
        yield arr, H, W


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("C", [8, 520, 1032, 2048, 2056])
def test_upsampler_fp16_vec8_windows(C, keep):
    """fp16 source, C % 8 == 0, aligned: k_upsample_hwc<_Float16, _Float16 | float, 8, NV> (voxproj.hip:807-809), NV from
    groups = ceil(C / 512) (VP_UPS, :793-800): 8 -> 1, 520 -> 2, 1032 -> 4 (3 groups), 2048 -> 4, 2056 -> 0 (5 groups: any C)."""
    for arr, H, W in _maps(C, np.float16, C + keep):
        _check_upsample(arr, H, W, keep)


@pytest.mark.parametrize("C", [4, 260, 772, 1024, 1028])
def test_upsampler_fp32_vec4_windows(C):
    """fp32 source, C % 4 == 0, aligned: k_upsample_hwc<float, float, 4, NV> (voxproj.hip:815), groups = ceil(C / 256):
    4 -> NV 1, 260 -> 2, 772 -> 4 (3 groups), 1024 -> 4, 1028 -> 0; the transpose k_chw_to_hwc_v16<float> for h*w % 4 == 0,
    k_chw_to_hwc<float> otherwise (:811-814)."""
    for arr, H, W in _maps(C, np.float32, C):
        _check_upsample(arr, H, W, False)


@pytest.mark.parametrize("dt,keep", [(np.float32, False), (np.float16, False), (np.float16, True)])
@pytest.mark.parametrize("C", [63, 65, 129, 257])
def test_upsampler_vec1_windows(C, dt, keep):
    """C % 4 != 0 (and so C % 8 != 0): the VEC = 1 arms (voxproj.hip:808-809,815), groups = ceil(C / 64): 63 -> NV 1, 65 -> 2,
    129 -> 4 (3 groups), 257 -> 0; transposes k_chw_to_hwc<float> / k_chw_to_hwc<_Float16>."""
    for arr, H, W in _maps(C, dt, C * 3 + keep):
        _check_upsample(arr, H, W, keep)


@pytest.mark.parametrize("dt,keep", [(np.float32, False), (np.float16, False), (np.float16, True)])
def test_upsampler_vec1_forced_by_a_misaligned_destination(dt, keep):
    """C = 512, but ``out`` (the aggregator passes pool slots, aggregate_voxel_features_onthefly.py:581) is a contiguous view one
    element off a 16-byte boundary: al16 is false (voxproj.hip:801) and the VEC = 1 arm runs with groups = 8 -> NV = 0:
    k_upsample_hwc<float, float, 1, 0>, <_Float16, _Float16, 1, 0>, <_Float16, float, 1, 0>.  Nothing around ``out`` is written."""
    for arr, H, W in _maps(512, dt, 17 + keep):
        _check_upsample(arr, H, W, keep, out_off=1)


@pytest.mark.parametrize("dt,C", [(np.float16, 520), (np.float32, 260)])
def test_upsampler_transposes_a_misaligned_source(dt, C):
    """A source that is a contiguous view one element off a 16-byte boundary takes the element-wise transpose k_chw_to_hwc<T>
    (voxproj.hip:803,811) even where h*w and C would allow the 16-byte one -- (4, 6) -> (9, 13) among the sizes."""
    for arr, H, W in _maps(C, dt, 29 + C):
        _check_upsample(arr, H, W, dt == np.float16, src_off=1)
