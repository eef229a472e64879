"""CPU tests of the text query: host-side refusals of vp_query_features (fake device pointers that are never dereferenced),
vp_query_workspace_bytes, the label palette, the .npz / .ply writers and the CLI's argument errors."""
import ctypes

import numpy as np
import pytest

import query_reference as qr

FAKE = 0x7000_0000_0000           # a "device" address: every call below is refused before any launch
WS = 0x7100_0000_0000             # 256-byte aligned


@pytest.fixture(scope="module")
def lib():
    import voxproj_host
    voxproj_host.build()
    return voxproj_host.lib()


def _call(lib, rows=FAKE, f16=1, n=100, C=512, stride=512, text=FAKE, P=13, scale=1.0, labels=FAKE, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.vp_query_workspace_bytes(P, C) if 1 <= P <= 1024 and 1 <= C <= 2048 else 1 << 30
    vp = ctypes.c_void_p
    return lib.vp_query_features(vp(rows), f16, n, C, stride, vp(text), P, scale, vp(FAKE), vp(labels), vp(FAKE), None,
                                 vp(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(rows=0), -1, b"null pointer"),
    (dict(labels=0), -1, b"null pointer"),
    (dict(text=0), -1, b"null pointer"),
    (dict(n=0), -1, b"n_rows"),
    (dict(n=-5), -1, b"n_rows"),
    (dict(n=1 << 31), -1, b"n_rows"),
    (dict(C=0, stride=0), -1, b"C = 0"),
    (dict(C=2049, stride=4096), -1, b"C = 2049"),
    (dict(P=0), -1, b"P = 0"),
    (dict(P=1025), -1, b"P = 1025"),
    (dict(stride=511), -1, b"row_stride"),
    (dict(scale=0.0), -1, b"scale"),
    (dict(scale=-1.0), -1, b"scale"),
    (dict(scale=float("inf")), -1, b"scale"),
    (dict(scale=float("nan")), -1, b"scale"),
    (dict(ws=0), -2, b"workspace"),
    (dict(ws_bytes=1024), -2, b"workspace has 1024 bytes"),
    (dict(ws=WS + 16), -2, b"256-byte aligned"),
])
def test_host_refusals(lib, kw, code, msg):
    assert _call(lib, **kw) == code
    assert msg in lib.vp_last_error()


def test_query_symbols_in_exports_and_header():
    import os
    import voxproj_host
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "voxproj.h")).read()
    for name in ("vp_query_workspace_bytes", "vp_query_features"):
        assert name in voxproj_host.EXPORTS and f" {name}(" in hdr
    assert voxproj_host.VP_ABI_VERSION == 4


def test_workspace_bytes_monotone(lib):
    prev = 0
    for P in (1, 2, 15, 16, 17, 100, 512, 1024):
        cur = [lib.vp_query_workspace_bytes(P, C) for C in (1, 7, 8, 31, 32, 33, 512, 768, 2048)]
        assert all(b > 0 and b % 256 == 0 for b in cur)
        assert cur == sorted(cur) and cur[0] >= prev
        prev = cur[0]
    # enough for the zero-padded f32 text table
    assert lib.vp_query_workspace_bytes(13, 512) >= 16 * 512 * 4
    assert lib.vp_query_workspace_bytes(1024, 2048) >= 1024 * 2048 * 4
    for P, C in ((0, 512), (1025, 512), (13, 0), (13, 2049)):
        assert lib.vp_query_workspace_bytes(P, C) == 0


def test_palette():
    import query_voxel_features as qvf
    pal = qvf.palette(300)
    assert pal.dtype == np.uint8 and pal.shape == (300, 3)
    assert tuple(pal[0]) == (0, 0, 0)
    assert tuple(pal[1]) == (128, 0, 0) and tuple(pal[2]) == (0, 128, 0) and tuple(pal[4]) == (0, 0, 128)
    assert tuple(pal[8]) == (64, 0, 0) and tuple(pal[3]) == (128, 128, 0) and tuple(pal[64]) == (32, 0, 0)
    assert np.array_equal(pal, qr.palette(300))
    assert len({tuple(c) for c in pal}) == 300                     # distinct colours
    cols = qvf.label_colors(np.array([2, -1, 1], np.int16), 5)
    assert np.array_equal(cols, np.array([[0, 128, 0], [0, 0, 0], [128, 0, 0]], np.uint8))


def test_writers(tmp_path):
    import query_voxel_features as qvf
    lab = np.array([0, 2, 1, -1], np.int32)
    lg = np.arange(12, dtype=np.float64).reshape(4, 3)
    cols = qvf.label_colors(lab, 3)
    qvf.write_npz(str(tmp_path / "x.npz"), lab, lg, ["a", "b", "c"], cols)
    z = np.load(tmp_path / "x.npz")
    assert z["labels"].dtype == np.int16 and z["labels"].tolist() == [0, 2, 1, -1]
    assert z["logits"].dtype == np.float32 and z["logits"].shape == (4, 3)
    assert list(z["prompts"]) == ["a", "b", "c"] and z["colors"].dtype == np.uint8 and z["colors"].shape == (4, 3)
    qvf.write_npz(str(tmp_path / "y.npz"), lab, lg, ["a", "b", "c"])
    assert "colors" not in np.load(tmp_path / "y.npz").files
    xyz = np.array([[0.5, 1.0, -2.0], [1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    qvf.write_ply(str(tmp_path / "x.ply"), xyz, cols)
    text = (tmp_path / "x.ply").read_text()
    header, body = text.split("end_header\n")
    assert header.startswith("ply\nformat ascii 1.0\nelement vertex 4\n")
    assert "property float x" in header and "property uchar red" in header and "property uchar blue" in header
    lines = body.splitlines()
    assert len(lines) == 4 and lines[0].split() == ["0.5", "1.0", "-2.0", "0", "0", "0"]
    assert lines[1].split()[3:] == ["0", "128", "0"]


def test_load_text(tmp_path):
    import torch
    import query_voxel_features as qvf
    t = np.random.default_rng(0).standard_normal((3, 8)).astype(np.float32)
    np.save(tmp_path / "t.npy", t)
    torch.save(torch.from_numpy(t), tmp_path / "t.pt")
    torch.save(torch.from_numpy(t).half(), tmp_path / "h.pt")
    torch.save({"text": torch.from_numpy(t)}, tmp_path / "d.pt")
    assert np.array_equal(qvf.load_text(str(tmp_path / "t.npy")).numpy(), t)
    assert np.array_equal(qvf.load_text(str(tmp_path / "t.pt")).numpy(), t)
    assert qvf.load_text(str(tmp_path / "h.pt")).dtype == torch.float32
    with pytest.raises(ValueError, match="one"):
        qvf.load_text(str(tmp_path / "d.pt"))
    np.save(tmp_path / "bad.npy", t[0])
    with pytest.raises(ValueError, match=r"\[P, C\]"):
        qvf.load_text(str(tmp_path / "bad.npy"))


def test_cli_argument_errors(tmp_path, capsys):
    import query_voxel_features as qvf
    np.save(tmp_path / "t.npy", np.ones((3, 8), np.float32))
    t = str(tmp_path / "t.npy")
    with pytest.raises(SystemExit):                                 # 2 prompts for 3 embedding rows
        qvf.main(["voxels", "--text_emb", t, "--prompt", "a", "b", "--vox", "x.pt", "--out", "x.npz"])
    assert "2 prompts for 3 embedding rows" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                 # gaussians without --gauss
        qvf.main(["gaussians", "--text_emb", t, "--prompt", "a", "b", "c", "--vox", "x.pt", "--out", "x.npz"])
    assert "--gauss" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        qvf.main(["voxels", "--text_emb", t, "--prompt", "a", "b", "c", "--vox", "x.pt", "--out", "x.npz", "--logit_scale", "0"])
    assert "logit_scale" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                 # no sub-command
        qvf.main(["--text_emb", t])


def test_reference_formula_basics():
    rows = np.array([[1.0, 0.0], [0.0, 0.0], [np.inf, 1.0], [1.0, 1.0]])
    text = np.array([[1.0, 0.0], [0.0, 2.0], [1.0, 0.0]])
    L, lab, m, bad = qr.query64(rows, text)
    assert lab.tolist() == [0, 0, -1, 0] and bad.tolist() == [False, False, True, False]
    assert m[1] == 0 and np.isnan(m[2]) and np.isclose(L[3, 1], np.sqrt(0.5))
    assert qr.bound(512) == pytest.approx(5.49e-4, rel=1e-2)
