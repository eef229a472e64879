"""vp_label_sums and vp_row_inv_norms on the GPU against tests/label_sums_reference.py: sums and counts equal the twin byte
for byte, and every element independently meets clause (F) of tests/sum_criteria.py against float64 sums that share nothing
with the twin's code path.  The shapes are the ones at which the kernels can go wrong, not the workload's: one row, one
wavefront of rows and one more, element-wise and 16-byte rows, one and several slots per lane, rows wider than one channel pass of every row variant, a ragged tail, the ninth key
bit, the largest K, every row its own part, ragged last parts, one part, the default."""
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

import label_sums_reference as ref  # noqa: E402
import sum_criteria  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def make_rows(N, C, dtype, layout, seed):
    """(tensor [N,C] on the GPU in the asked layout, the same values as a NumPy array).  Layouts: plain; wide (row stride
    C + 8: 16-byte loads stay possible when C allows them); odd (row stride C + 3: element loads); shifted (a base one
    element past a 16-byte boundary: element loads)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, C)).astype(dtype)
    t = torch.from_numpy(x)
    if layout == "plain":
        g = t.to(DEV)
    elif layout in ("wide", "odd"):
        big = torch.full((N, C + (8 if layout == "wide" else 3)), 77.0, dtype=t.dtype, device=DEV)
        big[:, :C] = t.to(DEV)
        g = big[:, :C]
    else:
        flat = torch.full((N * C + 16,), 77.0, dtype=t.dtype, device=DEV)
        assert flat.data_ptr() % 16 == 0
        g = flat[1:1 + N * C].view(N, C)
        g.copy_(t.to(DEV))
        assert g.data_ptr() % 16 != 0
    return g, x


def make_labels(N, K, kind, seed):
    rng = np.random.default_rng(seed + 1000)
    if kind == "random":
        lab = rng.integers(0, K, N)
    elif kind == "with_ignored":
        lab = np.where(rng.random(N) < 0.2, -1 - rng.integers(0, 3, N), rng.integers(0, K, N))
    elif kind == "one_label":
        lab = np.full(N, K - 1)
    elif kind == "all_ignored":
        lab = np.full(N, -1)
    elif kind == "sorted":
        lab = np.sort(rng.integers(0, K, N))
    elif kind == "reversed":
        lab = np.sort(rng.integers(0, K, N))[::-1].copy()
    else:
        raise KeyError(kind)
    return lab.astype(np.int32)


def run(g, lab, K, scale=None, part_rows=0, **kw):
    import voxproj_host
    s = None if scale is None else torch.from_numpy(scale).to(DEV)
    sums, counts, status = voxproj_host.label_sums(g, torch.from_numpy(lab).to(DEV), K, row_scale=s, part_rows=part_rows, check=False, **kw)
    return sums.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()


def compare(got, x, lab, K, scale, part_rows):
    """Byte equality with the twin; clause (F) against the float64 sums of the exact products."""
    sums, counts, status = got
    t_sums, t_counts, t_status = ref.label_sums(x, lab, K, scale, part_rows)
    assert counts.dtype == np.int32 and counts.tobytes() == t_counts.tobytes()
    assert status.tolist() == t_status.tolist()
    assert sums.dtype == np.float32 and sums.shape == (K, x.shape[1])
    differ = int((sums.view(np.uint32) != t_sums.view(np.uint32)).sum())
    assert differ == 0, f"{differ} element(s) differ from the twin's bits"
    ref64, abs64, n64 = ref.sums64(x, lab, K, scale)
    assert np.array_equal(n64, counts)
    err = np.abs(sums.astype(np.float64) - ref64)
    bound = sum_criteria.K_FWD * np.sqrt(n64.astype(np.float64))[:, None] * sum_criteria.U32 * abs64
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"(F) worst ratio {worst:.3f}; {int((n64 > 0).sum())} of {K} labels have rows, longest {int(n64.max())}")
    assert (err <= bound).all(), f"(F) worst ratio {worst:.3g}"
    assert not sums[n64 == 0].any()


# N, C, K, part_rows, dtype, rows' layout, labels, with a row scale
CASES = [
    (1, 7, 1, 0, np.float16, "plain", "random", False),
    (1, 512, 10, 1, np.float32, "plain", "random", True),
    (63, 8, 2, 1, np.float16, "plain", "random", True),
    (64, 40, 10, 3, np.float32, "plain", "with_ignored", False),
    (65, 512, 256, 64, np.float16, "plain", "random", False),
    (65, 8, 300, 3, np.float32, "wide", "random", True),
    (1000, 520, 300, 0, np.float16, "plain", "with_ignored", True),
    (1000, 7, 300, 1, np.float32, "plain", "random", False),
    (1000, 40, 10, 64, np.float16, "wide", "sorted", True),
    (1000, 40, 10, 3, np.float16, "odd", "reversed", False),
    (1000, 512, 2, 64, np.float16, "shifted", "random", True),
    (1000, 520, 10, 3, np.float32, "shifted", "with_ignored", False),
    (6000, 512, 10, 0, np.float16, "plain", "random", True),
    (6000, 520, 2, 0, np.float32, "plain", "with_ignored", True),
    (6000, 40, 65536, 3, np.float16, "plain", "random", False),
    (6000, 8, 65536, 0, np.float32, "plain", "one_label", True),
    (6000, 40, 1, 1, np.float16, "plain", "one_label", False),
    (6000, 7, 256, 64, np.float16, "plain", "sorted", True),
    (6000, 512, 300, 0, np.float32, "wide", "reversed", False),
    (1000, 8, 10, 0, np.float16, "plain", "all_ignored", False),
    (64, 520, 1, 0, np.float16, "odd", "one_label", True),
    # Rows wider than one channel pass of k_label_part_sums (64 * W * NS channels, NS = 4 above with_step's ladder: 1024 for
    # 16-byte fp32 rows, 2048 for 16-byte fp16 rows, 256 element-wise; tests/README_laps.md): the cases above take a second
    # pass in the element-wise variants only.
    (65, 1028, 4, 3, np.float32, "plain", "with_ignored", True),      # 1024 + 4: one active lane in the second pass
    (65, 2052, 3, 3, np.float32, "wide", "random", False),            # three passes, the third of one lane
    (65, 4096, 2, 3, np.float32, "plain", "random", True),            # CL_MAX_C: four full passes
    (1000, 2056, 10, 0, np.float16, "plain", "with_ignored", True),   # 2048 + 8, the default R
    (65, 4096, 4, 3, np.float16, "wide", "reversed", False),          # two full passes
    (65, 1025, 5, 3, np.float32, "shifted", "random", True),          # element-wise, five passes, the last of one lane
]


@pytest.mark.parametrize("N,C,K,part_rows,dtype,layout,labels,scaled", CASES,
                         ids=[f"N{c[0]}-C{c[1]}-K{c[2]}-R{c[3]}-{np.dtype(c[4]).name}-{c[5]}-{c[6]}-{'scaled' if c[7] else 'plain'}" for c in CASES])
def test_label_sums_equal_the_twin_bit_for_bit(N, C, K, part_rows, dtype, layout, labels, scaled):
    seed = N + C + K + part_rows
    g, x = make_rows(N, C, dtype, layout, seed)
    lab = make_labels(N, K, labels, seed)
    scale = np.random.default_rng(seed + 2000).uniform(0.25, 2.0, N).astype(np.float32) if scaled else None
    compare(run(g, lab, K, scale, part_rows), x, lab, K, scale, part_rows)


def test_the_default_part_size_cuts_a_long_label_and_the_cut_shows():
    """6000 float32 rows of one sign in one label (float16 values of one binade would add exactly in any order): with the
    default R = 256 the label is summed in 24 parts, which is not the one-part sum (so the parts are real), and each is the
    twin's."""
    rng = np.random.default_rng(5)
    x = rng.uniform(0.5, 1.0, (6000, 8)).astype(np.float32)
    g, lab = torch.from_numpy(x).to(DEV), np.zeros(6000, np.int32)
    a, b = run(g, lab, 1), run(g, lab, 1, part_rows=6000)
    compare(a, x, lab, 1, None, 0)
    compare(b, x, lab, 1, None, 6000)
    assert a[0].tobytes() != b[0].tobytes()
    assert run(g, lab, 1, part_rows=1 << 40)[0].tobytes() == b[0].tobytes()        # a part longer than the table is the whole label


def test_labels_out_of_range_are_counted_left_out_and_the_wrapper_raises():
    import voxproj_host
    g, x = make_rows(1000, 40, np.float16, "plain", 11)
    lab = make_labels(1000, 10, "with_ignored", 11)
    lab[::7] = 10                                     # the first label past the end
    lab[3::50] = 2 ** 31 - 1
    got = run(g, lab, 10)
    assert got[2].tolist() == [int((lab < 0).sum()), int((lab >= 10).sum())] and got[2][1] >= 143
    compare(got, x, lab, 10, None, 0)
    with pytest.raises(voxproj_host.VoxprojError, match=rf"{got[2][1]} row\(s\) carry a label >= K = 10"):
        voxproj_host.label_sums(g, torch.from_numpy(lab).to(DEV), 10)
    ok = voxproj_host.label_sums(g, torch.from_numpy(np.where(lab >= 10, -1, lab).astype(np.int32)).to(DEV), 10)       # check=True passes
    assert ok[0].cpu().numpy().tobytes() == got[0].tobytes()


def test_runs_are_bit_identical_also_on_a_side_stream_with_a_recycled_workspace():
    import voxproj_host
    g, x = make_rows(6000, 520, np.float16, "plain", 21)
    lab = make_labels(6000, 300, "with_ignored", 21)
    scale = np.random.default_rng(22).uniform(0.25, 2.0, 6000).astype(np.float32)
    first, second = run(g, lab, 300, scale, 64), run(g, lab, 300, scale, 64)
    ws = voxproj_host.SplatWorkspace()
    ws.ensure(voxproj_host.label_sums_workspace_bytes(6000, 300, 520, 64), DEV)
    ws.buf.fill_(255)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = run(g, lab, 300, scale, 64, workspace=ws)
        ws.buf.fill_(255)
        fourth = run(g, lab, 300, scale, 64, workspace=ws)      # the same buffer again, dirtied in between
    side.synchronize()
    for other in (second, third, fourth):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, other))
    compare(first, x, lab, 300, scale, 64)


def test_mask_pooling_shape():
    """The sums behind the mean feature per mask id of a 2D map: 64 x 48 pixels of a channels-last fp16 map, 300 ids of which
    the 4 x 4 blobs use 192 and a border is unlabelled."""
    rng = np.random.default_rng(31)
    fmap = rng.normal(size=(48, 64, 16)).astype(np.float16)
    yy, xx = np.mgrid[0:48, 0:64]
    ids = ((yy // 4) * 16 + xx // 4).astype(np.int32)
    ids[0, :] = -1
    ids[:, 63] = -1
    g = torch.from_numpy(fmap).to(DEV).view(48 * 64, 16)
    got = run(g, ids.reshape(-1), 300)
    compare(got, fmap.reshape(-1, 16), ids.reshape(-1), 300, None, 0)
    assert int((got[1] > 0).sum()) == 192 and got[2].tolist() == [48 + 64 - 1, 0]


# ---- vp_row_inv_norms ----
NORM_CASES = [(1, 7, np.float16, "plain"), (65, 8, np.float16, "plain"), (1000, 40, np.float16, "wide"), (1000, 40, np.float32, "plain"),
              (63, 128, np.float32, "plain"), (1000, 512, np.float16, "plain"), (64, 520, np.float16, "odd"), (1000, 512, np.float32, "shifted"),
              (65, 16, np.float32, "odd"), (6000, 32, np.float16, "plain")]


@pytest.mark.parametrize("N,C,dtype,layout", NORM_CASES, ids=[f"N{c[0]}-C{c[1]}-{np.dtype(c[2]).name}-{c[3]}" for c in NORM_CASES])
def test_row_inv_norms_within_one_ulp_and_bad_rows_counted(N, C, dtype, layout):
    import voxproj_host
    g, x = make_rows(N, C, dtype, layout, N + C)
    rng = np.random.default_rng(N * C)
    x = x * rng.uniform(0.01, 30.0, (N, 1)).astype(dtype)
    if N >= 63:
        x[5] = 0
        x[17, C // 2] = np.inf
        x[18, C - 1] = np.nan
        x[40] = 0
        x[41] = 0
        x[41, C - 1] = 6e-8 if dtype == np.float16 else 1e-42         # one subnormal element: not a zero row
        x[42] = 6e-8 if dtype == np.float16 else 1e-42                # a subnormal row
    g.copy_(torch.from_numpy(x).to(DEV))
    inv, status = voxproj_host.row_inv_norms(g)
    inv, status = inv.cpu().numpy(), status.cpu().numpy()
    inv64, zero, bad = ref.inv_norms64(x)
    assert inv.dtype == np.float32 and status.tolist() == [int(zero.sum()), int(bad.sum())] == ([2, 2] if N >= 63 else [0, 0])
    assert not inv[zero | bad].any() and (inv[~(zero | bad)] > 0).all()
    ulp = np.spacing(inv64.astype(np.float32)).astype(np.float64)
    worst = float((np.abs(inv.astype(np.float64) - inv64) / ulp).max())
    print(f"worst error {worst:.3f} ulp of float32")
    assert worst <= 1.0
    if N >= 63:
        with pytest.raises(voxproj_host.VoxprojError, match=r"2 all-zero row\(s\) and 2 row\(s\) with a non-finite element"):
            voxproj_host.row_inv_norms(g, check=True)
