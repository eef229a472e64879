"""CPU-side checks of the projector's transpose (vp_first_hit_ids, vp_render_features) and of its Python layer: the symbols
are exported and declared, every documented refusal is decided on the host (the "device" pointers here are fakes that are
never dereferenced), and the Python entry points refuse CPU tensors and wrong dtypes before any library call."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x7000_0000_0000          # fake "device" addresses, 256-byte aligned


def test_transpose_symbols_are_exported_and_declared():
    import voxproj_host
    voxproj_host.build()
    lib = ctypes.CDLL(voxproj_host.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "voxproj.h")).read()
    for name in ("vp_first_hit_ids", "vp_render_features"):
        assert hasattr(lib, name), name
        assert name in voxproj_host.EXPORTS, name
        assert f"int {name}(" in hdr, name
    assert voxproj_host.lib().vp_abi_version() == 4          # new symbols, same ABI version


def _first_hit_call(lib, **kw):
    o = (ctypes.c_float * 5)(48, 32, 0.01, 10.0, 0.05)
    g = (ctypes.c_float * 3)(0, 0, 0)
    a = dict(occ=P + 4096, vmi=P + 8192, intr=P + 12288, opts=o, origin=g, vs=0.1, B=1, V=2, H=32, W=48, dz=10, dy=20, dx=30,
             n_rows=1001, ids=P + 16384, ws=P + (1 << 20), ws_bytes=1 << 30, stream=None, flags=0)
    a.update(kw)
    return lib.vp_first_hit_ids(a["occ"], a["vmi"], a["intr"], a["opts"], a["origin"], ctypes.c_float(a["vs"]), a["B"], a["V"],
                                a["H"], a["W"], a["dz"], a["dy"], a["dx"], a["n_rows"], a["ids"], a["ws"], a["ws_bytes"],
                                a["stream"], a["flags"])


def test_first_hit_ids_validates_its_arguments_before_touching_the_device():
    import voxproj_host as vh
    lib = vh.lib()
    cases = [
        (dict(flags=vh.VP_FLAG_PIPELINE), -1, b"accepts VP_FLAG_SYNC"),
        (dict(flags=vh.VP_FLAG_GATHER_ONLY), -1, b"accepts VP_FLAG_SYNC"),
        (dict(flags=vh.VP_FLAG_SERIAL_SUMS | vh.VP_FLAG_SYNC), -1, b"accepts VP_FLAG_SYNC"),
        (dict(flags=1 << 12), -1, b"accepts VP_FLAG_SYNC"),
        (dict(ids=None), -1, b"null pointer"), (dict(occ=None), -1, b"null pointer"), (dict(vmi=None), -1, b"null pointer"),
        (dict(intr=None), -1, b"null pointer"), (dict(ws=None), -1, b"null pointer"),
        (dict(V=0), -1, b"non-positive"), (dict(n_rows=0), -1, b"non-positive"), (dict(dz=-1), -1, b"non-positive"),
        (dict(B=256, V=257), -1, b"exceeds 65535"),
        (dict(dz=2048, dy=1024, dx=1024), -1, b"2^31 cells"),
        (dict(opts=(ctypes.c_float * 5)(47, 32, 0.01, 10.0, 0.05)), -1, b"must equal the feature map"),
        (dict(opts=(ctypes.c_float * 5)(48, 31, 0.01, 10.0, 0.05)), -1, b"must equal the feature map"),
        (dict(opts=(ctypes.c_float * 5)(48, 32, 0.01, 10.0, 0.0)), -1, b"rayIncrement must be > 0"),
        (dict(opts=(ctypes.c_float * 5)(48, 32, 0.01, 10.0, float("nan"))), -1, b"rayIncrement must be > 0"),
        (dict(ws_bytes=4096), -2, b"need"), (dict(ws=P + (1 << 20) + 16), -2, b"256-byte aligned"),
    ]
    for kw, rc, msg in cases:
        assert _first_hit_call(lib, **kw) == rc, kw
        assert msg in lib.vp_last_error(), (kw, lib.vp_last_error())
    # the workspace it needs is vp_workspace_bytes(..., C = 1, ...): one byte less is refused
    need = vh.workspace_bytes(1, 2, 32, 48, 1, 10, 20, 30, 1001)
    assert _first_hit_call(lib, ws_bytes=need - 1) == -2 and b"need" in lib.vp_last_error()


def test_render_features_validates_its_arguments_before_touching_the_device():
    import voxproj_host as vh
    lib = vh.lib()

    def call(**kw):
        a = dict(ids=P, n_pixels=1000, rows=P + 65536, n_rows=10, C=8, dst=P + (1 << 20), f16=0, bad=None, stream=None)
        a.update(kw)
        return lib.vp_render_features(a["ids"], a["n_pixels"], a["rows"], a["n_rows"], a["C"], a["dst"], a["f16"], a["bad"],
                                      a["stream"])
    cases = [
        (dict(ids=None), b"null pointer"), (dict(rows=None), b"null pointer"), (dict(dst=None), b"null pointer"),
        (dict(n_pixels=0), b"non-positive"), (dict(n_pixels=-5), b"non-positive"), (dict(n_rows=0), b"non-positive"),
        (dict(C=0), b"non-positive"), (dict(C=-1), b"non-positive"), (dict(C=0, f16=1), b"non-positive"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.vp_last_error(), (kw, lib.vp_last_error())


def _no_library_calls(monkeypatch):
    """Any library call from here on fails the test."""
    import voxproj_host

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(voxproj_host, "lib", boom)


def test_python_entry_points_refuse_cpu_tensors_and_wrong_dtypes_before_any_library_call(monkeypatch):
    import project_features_autograd as pfa
    import voxproj_host
    _no_library_calls(monkeypatch)
    ids = torch.zeros(1, 1, 4, 4, dtype=torch.int32)
    rows = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="CUDA tensor"):
        voxproj_host.render_features(ids, rows)
    with pytest.raises(ValueError, match="must be torch.int32"):
        voxproj_host.render_features(ids.long(), rows)
    with pytest.raises(ValueError, match="must be torch.float32"):
        voxproj_host.render_features(ids, rows.double())
    with pytest.raises(ValueError, match="dtype must be"):
        voxproj_host.render_features(ids, rows, dtype=torch.bfloat16)
    occ = torch.zeros(1, 2, 2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="CUDA tensor"):
        voxproj_host.first_hit_ids(occ, torch.zeros(16), torch.zeros(1, 4), [4, 4, 0.01, 10.0, 0.5], [0, 0, 0], 1.0, 4, 4, 3)
    with pytest.raises(ValueError, match="must be torch.int64"):
        voxproj_host.first_hit_ids(occ.int(), torch.zeros(16), torch.zeros(1, 4), [4, 4, 0.01, 10.0, 0.5], [0, 0, 0], 1.0, 4, 4, 3)
    feats = torch.zeros(1, 1, 4, 4, 8, requires_grad=True)
    args = (occ, torch.zeros(16), torch.zeros(1, 4), [4, 4, 0.01, 10.0, 0.5], [0, 0, 0], 1.0, 3)
    with pytest.raises(ValueError, match="CUDA tensor"):
        pfa.project_features(feats, *args)
    with pytest.raises(ValueError, match="float32 or float16"):
        pfa.project_features(feats.detach().double(), *args)
    with pytest.raises(ValueError, match="reduce"):
        pfa.project_features(feats, *args, reduce="max")


def test_autograd_entry_refuses_mismatched_shapes_before_any_library_call(monkeypatch):
    """The library takes B, V, H, W, C from the feature maps and only the grid's dims from occ: every shape that would make the
    device read past occ, vmi or intr is refused in Python first (CPU tensors: the shape checks come before the device check)."""
    import project_features_autograd as pfa
    _no_library_calls(monkeypatch)
    B, V, H, W, C = 2, 3, 4, 6, 8
    feats = torch.zeros(B, V, H, W, C, requires_grad=True)
    occ = torch.zeros(B, 2, 2, 2, dtype=torch.int64)
    vmi = torch.zeros(B * V * 16)
    intr = torch.zeros(B, 4)
    opts = [W, H, 0.01, 10.0, 0.5]

    def call(**kw):
        a = dict(feats=feats, occ=occ, vmi=vmi, intr=intr, opts5=opts, grid_origin3=[0, 0, 0], voxel_size=1.0, n_rows=3)
        a.update(kw)
        return pfa.project_features(**a)
    cases = [
        (dict(occ=torch.zeros(1, 2, 2, 2, dtype=torch.int64)), "occ must be \\[B,Z,Y,X\\] with B = 2"),     # one grid for two batches
        (dict(occ=torch.zeros(B, 2, 2, dtype=torch.int64)), "occ must be"),
        (dict(occ=torch.zeros(B, 0, 2, 2, dtype=torch.int64)), "occ must be"),
        (dict(vmi=torch.zeros((B * V - 1) * 16)), "vmi must hold B\\*V\\*16 = 96"),                        # a view short
        (dict(vmi=torch.zeros(B, V + 1, 4, 4)), "vmi must hold"),
        (dict(intr=torch.zeros(1, 4)), "intr must be \\[B,4\\] with B = 2"),
        (dict(intr=torch.zeros(B, 3)), "intr must be"),
        (dict(intr=torch.zeros(4, 2)), "intr must be"),
        (dict(opts5=opts[:4]), "opts5 must hold 5 values"),
        (dict(opts5=[W + 1, H, 0.01, 10.0, 0.5]), "width/height"),
        (dict(grid_origin3=[0, 0]), "grid_origin3 must hold 3"),
        (dict(n_rows=0), "n_rows must be"),
        (dict(feats=torch.zeros(B, V, H, W, 0)), "every dimension"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="CUDA tensor"):          # well-formed CPU arguments reach the device check, and stop there
        call()
    with pytest.raises(ValueError, match="opts5 must hold 5 values"):
        import voxproj_host
        voxproj_host.first_hit_ids(occ, vmi, intr, opts[:4], [0, 0, 0], 1.0, H, W, 3)


def test_render_script_parses_its_command_line_and_refuses_to_run_without_a_gpu(monkeypatch):
    import render_voxel_features
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        render_voxel_features.main(["--features_pt", "x.pt", "--views", "a", "b"])
    with pytest.raises(SystemExit):
        render_voxel_features.main([])          # --features_pt is required
