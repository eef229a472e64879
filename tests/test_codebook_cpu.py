"""The code book of global instance labels without a GPU: the library's three symbols and their host-side refusals, the
workspace size function, the Python wrappers' argument checks, the linear assignment, the command line's argument errors,
the float64 reference's closed form against its own autograd, and the cap on fragile pixels for every case the GPU test
runs.  Everything that touches the library fails on a tree without vp_codebook_assoc."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-semantic-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import codebook_reference as cref  # noqa: E402
import proto_loss_reference as pref  # noqa: E402
import voxproj_host  # noqa: E402

SYMBOLS = ("vp_codebook_workspace_bytes", "vp_codebook_assoc", "vp_codebook_loss")
EINVAL, EWORKSPACE = -1, -2                              # VP_EINVAL, VP_EWORKSPACE of include/voxproj.h
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_three_symbols():
    L = voxproj_host.lib()
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for name in SYMBOLS:
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
        assert hasattr(L, name), f"libvoxproj.so has no {name}"
    assert L.vp_abi_version() == voxproj_host.VP_ABI_VERSION == 4       # detected by symbol: the version did not move
    assert "#define VP_CODEBOOK_MAX_CODES 256" in hdr and voxproj_host.VP_CODEBOOK_MAX_CODES == cref.MAX_CODES == 256
    assert "take no part" in hdr                                         # the deliberate difference is stated


def test_workspace_size_function():
    size = voxproj_host.codebook_workspace_bytes
    for D, K, W, H in [(0, 4, 5, 5), (65, 4, 5, 5), (-1, 4, 5, 5), (16, 0, 5, 5), (16, 257, 5, 5), (16, -1, 5, 5), (16, 4, 0, 5),
                       (16, 4, 5, 0), (16, 4, -1, 5), (16, 4, 32769, 1), (16, 4, 1, 32769)]:
        assert size(D, K, W, H) == 0
    for D, K in ((1, 1), (3, 5), (16, 256), (17, 17), (64, 256)):
        last = 0
        for W, H in [(1, 1), (16, 16), (37, 19), (130, 67), (145, 113), (1600, 1067), (32768, 32768)]:
            b = size(D, K, W, H)
            tiles = (W * H + 63) // 64
            groups = min(tiles, 256)
            assert b > 0 and b % 256 == 0 and b >= last and groups <= 256
            assert b >= groups * (256 * K * 4 + 2 * K * D * 4)           # a score table and two gradient sums per workgroup
            assert b <= groups * (1024 * K + 2048 + 8 * K * D + 256) + 6 * 256   # the header's statement
            last = b
    assert size(16, 256, 1600, 1067) <= 80 * 2 ** 20
    assert size(64, 256, 130, 67) > size(16, 256, 130, 67) > size(16, 16, 130, 67)


def _fake_buffers(nbytes):
    buf = ctypes.create_string_buffer(nbytes + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255            # never dereferenced: every call below is refused before a launch
    return buf, ws


def test_assoc_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    need = voxproj_host.codebook_workspace_bytes(16, 8, 8, 4)
    buf, ws = _fake_buffers(need)
    order = ("image", "D", "W", "H", "ids", "ignore_id", "codebook", "K", "score", "id_pixels", "pred", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, D=16, W=8, H=4, ids=ws, ignore_id=-1, codebook=ws, K=8, score=ws, id_pixels=ws, pred=None, ws=ws,
                 ws_bytes=need)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_codebook_assoc(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(codebook=None)), (EINVAL, dict(score=None)),
                     (EINVAL, dict(id_pixels=None)), (EINVAL, dict(D=0)), (EINVAL, dict(D=65)), (EINVAL, dict(K=0)),
                     (EINVAL, dict(K=257)), (EINVAL, dict(W=0)), (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)),
                     (EINVAL, dict(H=32769)), (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws=ws + 16)),
                     (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_loss_call_host_side_refusals_need_no_gpu():
    L = voxproj_host.lib()
    need = voxproj_host.codebook_workspace_bytes(16, 8, 8, 4)
    buf, ws = _fake_buffers(need)
    order = ("image", "D", "W", "H", "ids", "ignore_id", "conf", "conf_min", "codebook", "K", "assign", "stats", "grad_cls",
             "grad_cluster", "pixel_loss", "ws", "ws_bytes")

    def call(**over):
        a = dict(image=ws, D=16, W=8, H=4, ids=ws, ignore_id=-1, conf=None, conf_min=0.2, codebook=ws, K=8, assign=ws, stats=ws,
                 grad_cls=ws, grad_cluster=ws, pixel_loss=None, ws=ws, ws_bytes=need)
        assert set(over) <= set(a), over
        a.update(over)
        return L.vp_codebook_loss(*[a[k] for k in order], None)

    for rc, over in [(EINVAL, dict(image=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(codebook=None)), (EINVAL, dict(assign=None)),
                     (EINVAL, dict(stats=None)), (EINVAL, dict(grad_cls=None)), (EINVAL, dict(grad_cluster=None)),
                     (EINVAL, dict(D=0)), (EINVAL, dict(D=65)), (EINVAL, dict(K=0)), (EINVAL, dict(K=257)), (EINVAL, dict(W=0)),
                     (EINVAL, dict(W=32769)), (EINVAL, dict(H=0)), (EINVAL, dict(H=32769)), (EINVAL, dict(conf_min=NAN)),
                     (EINVAL, dict(conf_min=INF)), (EINVAL, dict(conf_min=-INF)), (EWORKSPACE, dict(ws=None)),
                     (EWORKSPACE, dict(ws=ws + 16)), (EWORKSPACE, dict(ws_bytes=need - 1))]:
        assert call(**over) == rc, over
        assert voxproj_host.last_error()
    assert buf.raw == bytes(len(buf)), "a refused call wrote into its buffers"


def test_python_wrappers_check_their_arguments_before_the_gpu():
    import splat_autograd
    img = torch.zeros((4, 3, 5), dtype=torch.float32)
    ids = torch.zeros((3, 5), dtype=torch.int32)
    cb = torch.zeros((6, 4), dtype=torch.float32)
    asg = torch.zeros(256, dtype=torch.int32)
    with pytest.raises(ValueError):
        voxproj_host.codebook_assoc(img.double(), ids, cb)
    with pytest.raises(ValueError):
        voxproj_host.codebook_assoc(img, ids.long(), cb)
    with pytest.raises(ValueError):
        voxproj_host.codebook_assoc(img, ids, cb[:, :3])                      # D of the code book
    with pytest.raises(ValueError):
        voxproj_host.codebook_assoc(img, ids, torch.zeros((257, 4)))
    with pytest.raises(ValueError):
        voxproj_host.codebook_assoc(img, ids, cb.double())
    with pytest.raises(ValueError):
        splat_autograd.codebook_loss(img.requires_grad_(), ids, None, cb, asg)


def test_assign_view_ids():
    g = np.random.default_rng(0)
    # fewer ids than codes: every present id gets the code where its score is largest (a permuted diagonal)
    K = 8
    score = g.uniform(0.0, 0.1, (256, K))
    px = np.zeros(256, np.int64)
    present = [3, 40, 41, 200, 255]
    want = [5, 0, 7, 2, 1]
    for l, k in zip(present, want):
        px[l] = 10 + l
        score[l, k] = 5.0
    score[100, 4] = 99.0                                                     # an absent id: its score must not matter
    a = voxproj_host.assign_view_ids(score, px, K)
    assert a.dtype == np.int32 and a.shape == (256,)
    assert [int(a[l]) for l in present] == want and (np.delete(a, present) == -1).all()
    # the optimum, not the greedy choice: id 1 prefers code 0 slightly, id 2 strongly
    s2 = np.zeros((256, 2))
    s2[1] = [1.0, 0.9]
    s2[2] = [1.0, 0.0]
    p2 = np.zeros(256, np.int64)
    p2[[1, 2]] = 5
    a = voxproj_host.assign_view_ids(s2, p2, 2)
    assert a[1] == 1 and a[2] == 0
    # more ids than codes: the first K in ascending order are kept, each with its own code
    K = 3
    score = g.uniform(0.0, 1.0, (256, K))
    px = np.zeros(256, np.int64)
    px[[9, 7, 250, 30, 8]] = 1
    a = voxproj_host.assign_view_ids(torch.from_numpy(score), torch.from_numpy(px), K)
    assert sorted(int(a[l]) for l in (7, 8, 9)) == [0, 1, 2] and a[30] == -1 and a[250] == -1 and (a >= 0).sum() == 3
    # no ids at all
    assert (voxproj_host.assign_view_ids(score, np.zeros(256, np.int64), K) == -1).all()
    with pytest.raises(ValueError):
        voxproj_host.assign_view_ids(score, px, K + 1)


def test_command_line_argument_errors(tmp_path):
    import associate_instances as ai
    assert ai.CONFIDENCE_PARAMS == pref.CONFIDENCE_PARAMS
    base = ["--gaussians_ply", "x.ply", "--cam_params", "c.json", "--masks_dir", str(tmp_path), "--gauss_feats", "i.pt", "--out",
            str(tmp_path / "o.pt")]
    for extra in (["--codes", "0"], ["--codes", "257"], ["--steps", "-1"], ["--lr", "0"], ["--lr", "nan"], ["--conf_min", "inf"],
                  ["--weight_cls", "nan"], ["--principal_point", "corner"]):
        with pytest.raises(SystemExit):
            ai.main(base + extra)
    for missing in ("--gauss_feats", "--out", "--masks_dir"):
        i = base.index(missing)
        with pytest.raises(SystemExit):
            ai.main(base[:i] + base[i + 2:])
    args = ai.build_parser().parse_args(base)
    assert (args.codes, args.steps, args.lr, args.conf_min, args.ignore_id, args.seed) == (256, 500, 5e-4, 0.2, -1, 0)
    cb = ai.init_codebook(256, 16, torch.Generator().manual_seed(0))
    assert cb.shape == (256, 16) and cb.dtype == torch.float32 and float(cb.abs().max()) <= 0.25 and float(cb.abs().max()) > 0.24
    assert torch.equal(cb, ai.init_codebook(256, 16, torch.Generator().manual_seed(0)))


def _small_case(seed, **kw):
    a = dict(D=5, K=7, W=20, H=20, layout="37", seed=seed, conf_kind="mixed", assign_kind="some")
    a.update(kw)
    return cref.make_case(**a)


@pytest.mark.parametrize("kind", ["mixed-some", "null-perm", "edge", "ties"])
def test_closed_form_equals_autograd_in_float64(kind):
    kw = {"mixed-some": {}, "null-perm": dict(conf_kind="null", assign_kind="perm"),
          "edge": dict(layout="edge", W=30, H=20, K=16, assign_kind="identity"), "ties": dict(ties=True, conf_kind="null")}[kind]
    image, ids, codebook, assign, conf = _small_case(3, **kw)
    ref = cref.statement64(image, ids, codebook, assign, conf, ignore_id=cref.IGNORE, want_grad=True)
    cf = cref.closed_form(image, ids, codebook, assign, conf, ignore_id=cref.IGNORE)
    assert ref["stats"][2] > 20 and np.abs(ref["grad_cls"]).max() > 1e-3 and np.abs(ref["grad_cluster"]).max() > 1e-3
    for key in ("score", "grad_cls", "grad_cluster", "pixel_loss"):
        assert np.abs(ref[key] - cf[key]).max() <= 1e-12 * max(np.abs(ref[key]).max(), 1.0), key
    assert np.allclose(ref["stats"], cf["stats"], rtol=1e-13, atol=0)
    assert (ref["id_pixels"] == cf["id_pixels"]).all() and (ref["pred"] == cf["pred"]).all()
    # what takes no part: exact zeros; the score rows of absent ids too; a row's mass is its pixel count
    assert not ref["pixel_loss"][~ref["part"]].any() and not ref["score"][ref["id_pixels"] == 0].any()
    assert np.allclose(ref["score"].sum(1), ref["id_pixels"], rtol=1e-12)
    assert (ref["pred"][~ref["valid"]] == -1).all()
    if kind == "ties":
        assert (ref["pred"] == 0).sum() > 20 and not (ref["pred"] == 1).any()       # the lowest of two equal logits
        assert cref.fragile_share(ref) <= 0.01                                       # an exact tie is not fragile
    # another order of pixels and channels is the same statement
    other = cref.closed_form(image, ids, codebook, assign, conf, ignore_id=cref.IGNORE, order=np.arange(400 if kind != "edge" else 600)[::-1],
                             chan=np.arange(5)[::-1])
    for key in ("score", "grad_cls", "grad_cluster", "pixel_loss"):
        assert np.abs(other[key] - cf[key]).max() <= 1e-11 * max(np.abs(cf[key]).max(), 1.0), key


def test_unassigned_ids_take_no_part():
    """More ids than codes: the pixels of an id without a code add nothing to the loss, its gradients or the mismatches."""
    image, ids, codebook, assign, conf = _small_case(4, K=3, conf_kind="null", assign_kind="identity")
    ref = cref.statement64(image, ids, codebook, assign, None, want_grad=True)
    assert (assign >= 0).sum() == 3 and len(np.unique(ids)) > 3
    keep = np.isin(ids, np.flatnonzero(assign >= 0))
    only = np.where(keep, ids, -1).astype(np.int32)
    ref2 = cref.statement64(image, only, codebook, assign, None, want_grad=True)
    assert ref["stats"] == ref2["stats"] and ref["stats"][2] == keep.sum()
    assert np.array_equal(ref["grad_cls"], ref2["grad_cls"]) and np.array_equal(ref["grad_cluster"], ref2["grad_cluster"])


def test_float32_yardstick_is_small_and_positive():
    image, ids, codebook, assign, conf = _small_case(3)
    b = cref.bounds(image, ids, codebook, assign, conf, ignore_id=cref.IGNORE)
    ref = cref.statement64(image, ids, codebook, assign, conf, ignore_id=cref.IGNORE)
    for key in cref.SUMS:
        assert 0 < b["E"][key] < 1e-3 and b[key] == 8 * b["E"][key]       # a non-zero yardstick is not raised by any floor
    assert b["score"] < 1e-4 * ref["score"].max()
    pb = cref.pixel_bound(ref)
    assert (pb > 0).all() and (pb < 1e-4).all()


@pytest.mark.parametrize("case", cref.shape_cases(), ids=cref.case_name)
def test_gpu_cases_stay_under_the_cap_on_fragile_pixels(case):
    image, ids, codebook, assign, conf = cref.make_case(**case)
    ref = cref.statement64(image, ids, codebook, assign, conf, ignore_id=cref.IGNORE)
    assert cref.fragile_share(ref) <= 0.01


def test_float64_training_reaches_the_end_condition():
    """tests/codebook_scene.py's loop, the command line's five steps in float64 on the CPU, reaches the discrete end
    condition in the STEPS = 150 steps the GPU test gives the command line: every view maps every class to one and the same
    code, no two classes to the same one."""
    import codebook_scene as cs
    scene = cs.make()
    for ids in scene["masks"]:
        assert len(np.unique(ids[ids >= 0])) == cs.CLASSES               # every class is seen in every view
    assert cs.STEPS == 150
    _, l0, l1, assigns = cs.train64(scene)
    table = cs.class_to_code(scene, assigns)
    print(l0, l1, table)
    assert l1 < l0 and cs.consistent(table)
    assert not cs.consistent(np.array([[0, 1, 2, 3], [0, 1, 3, 2]])) and not cs.consistent(np.array([[0, 1, 1, 3]]))
