"""Feature maps on which every float32 summation order leaves the same bytes, and the integer reference for them.

Every map value is a small integer.  While count * max|value| of a voxel stays below 2^24, every partial sum of any subset of its
pixels is an integer below 2^24 in magnitude: float32 holds it exactly, every addition is exact, and the serial wavefront, parts
added in slot order, the LDS meet, a whole-image redo, fp16 maps widened on load and accumulation across calls must all leave
the bytes of the int64 scatter-add cast to float32.  No tolerance is needed, and a difference is an integer that names its pixel:
the first four channels of a map are 1, x, y and v + 1, so a row that lacks (or doubles) one pixel differs from the reference by
-(1, x, y, v + 1) (or +) in channels 0..3.

Plain numpy; nothing of the package is imported."""
import numpy as np

VALUE_MAX = 1023            # exact in binary16 (11 significand bits) as well
CODE_CHANNELS = 4           # 1, x, y, v + 1
_CHUNK = 1024               # channels per np.add.at call (bounds the int64 temporaries of wide rows)


def exact_maps(V, H, W, C, seed, dtype=np.float32):
    """[V, H, W, C] maps of integers: channels 0..3 = 1, x, y, v + 1 for C >= 4, every other channel rng.integers(-64, 65);
    |value| <= 1023, so float16 maps hold the same numbers.  Zero is +0."""
    assert W - 1 <= VALUE_MAX and H - 1 <= VALUE_MAX and V <= VALUE_MAX, "the pixel code must fit |value| <= 1023"
    rng = np.random.default_rng(seed)
    m = rng.integers(-64, 65, size=(V, H, W, C), dtype=np.int16)
    if C >= CODE_CHANNELS:
        m[..., 0] = 1
        m[..., 1] = np.arange(W, dtype=np.int16)[None, None, :]
        m[..., 2] = np.arange(H, dtype=np.int16)[None, :, None]
        m[..., 3] = np.arange(1, V + 1, dtype=np.int16)[:, None, None]
    assert int(np.abs(m).max()) <= VALUE_MAX
    return m.astype(dtype)                      # integer 0 converts to +0


def int_reference(hits, maps, n_rows):
    """``hits``: int [B, V, H, W] first-hit IDs (0 = no hit); ``maps``: [B, V, H, W, C] or, for B == 1, [V, H, W, C].
    Returns (int64 [n_rows, C] scatter-add of every hit pixel's row with row 0 zeroed, int64 [n_rows] pixels per row).
    Integer arithmetic only."""
    ids = np.asarray(hits).reshape(-1).astype(np.int64)
    C = maps.shape[-1]
    rows = np.asarray(maps).reshape(-1, C)
    assert rows.shape[0] == ids.shape[0], (maps.shape, np.shape(hits))
    assert ids.min() >= 0 and ids.max() < n_rows
    ref = np.zeros((n_rows, C), np.int64)
    for c0 in range(0, C, _CHUNK):
        chunk = rows[:, c0:c0 + _CHUNK]
        as_int = chunk.astype(np.int64)
        assert np.array_equal(as_int, chunk), "the maps are not integers"
        np.add.at(ref[:, c0:c0 + _CHUNK], ids, as_int)
    ref[0] = 0
    count = np.bincount(ids, minlength=n_rows).astype(np.int64)
    count[0] = 0
    return ref, count


def assert_headroom(count_total, maps):
    """The condition of "any order, same bits": the largest row's pixel count (over ALL calls that add into one ``out``, from the
    oracle's counts) times the largest |value| stays below 2^24."""
    biggest = max(abs(float(np.max(maps))), abs(float(np.min(maps))))          # abs(maps).max() without a copy of wide maps
    assert np.isfinite(biggest)
    worst = int(np.max(count_total)) * int(np.ceil(biggest))
    assert worst < 2 ** 24, f"no headroom: {int(np.max(count_total))} pixels x |value| {biggest:g} = {worst} >= 2^24"


def _as_int(x):
    return int(x) if np.isfinite(x) and x == np.rint(x) else float(x)


def assert_exact(got_f32, ref_i64, count, label, split=None, max_rows=6):
    """``got_f32`` must hold the bytes of ``ref_i64`` cast to float32.  Otherwise AssertionError naming, for the first differing
    rows: the row ID, its pixel count, whether ``split`` (bool per row) marks it, got - ref of channels 0..3, how many channels
    differ, and -- when channel 0 differs by exactly one -- the pixel (v, y, x) the row lacks or holds twice."""
    got = np.ascontiguousarray(got_f32)
    assert got.dtype == np.float32 and got.shape == ref_i64.shape, (got.dtype, got.shape, ref_i64.shape)
    want = ref_i64.astype(np.float32)
    if got.tobytes() == want.tobytes():
        return
    differs = got.view(np.uint32) != want.view(np.uint32)
    rows = np.nonzero(differs.any(axis=1))[0]
    C = got.shape[1]
    lines = [f"{label}: {len(rows)} of {got.shape[0]} rows differ from the int64 scatter-add"]
    for i in rows[:max_rows]:
        d = got[i].astype(np.float64) - ref_i64[i].astype(np.float64)
        d4 = [_as_int(v) for v in d[:min(C, CODE_CHANNELS)]]
        mark = "n/a" if split is None else bool(split[i])
        line = (f"  row {int(i)}: {int(count[i])} pixels, split={mark}, got - ref of channels 0..{len(d4) - 1} = {d4}, "
                f"{int(differs[i].sum())} of {C} channels differ")
        if C >= CODE_CHANNELS and d4[0] in (1, -1) and all(isinstance(v, int) for v in d4):
            sign = d4[0]
            what = "holds twice" if sign > 0 else "lacks"
            line += f"; the row {what} pixel (v, y, x) = ({sign * d4[3] - 1}, {sign * d4[2]}, {sign * d4[1]})"
        lines.append(line)
    if len(rows) > max_rows:
        lines.append(f"  ... and rows {[int(i) for i in rows[max_rows:max_rows + 20]]}")
    raise AssertionError("\n".join(lines))
