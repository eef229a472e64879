"""tests/exact_maps.py without a GPU: the integer reference against the oracle, the premise (any float32 order, same bytes), and the
diagnosis assert_exact gives.  tests/test_gpu_exact_sums.py holds every role of the gather to this reference byte for byte."""
import numpy as np
import pytest

from exact_maps import assert_exact, assert_headroom, exact_maps, int_reference
from synthetic_scene import make_scene

ROOM = (5.0, 4.0, 2.4)
# (views, width, height, C): the scene of the redo tests, the same with nine views and ragged scalar rows, and one 640 x 416 view
# whose largest voxel collects ten thousand pixels
SCENES = {"six_views": (6, 48, 32, 12), "nine_views": (9, 48, 32, 259), "one_large_view": (1, 640, 416, 8)}
_cache = {}


def _case(oracle_mod, name):
    """Scene, maps, the oracle's call on them (hits, count, float32 out) and the integer reference; computed once."""
    if name not in _cache:
        V, W, H, C = SCENES[name]
        s = make_scene(2000, V, W, H, seed=71, room=ROOM)
        maps = exact_maps(V, H, W, C, seed=72)
        n_rows = s.n_vox + 1
        count, out = np.zeros(n_rows, np.int32), np.zeros((n_rows, C), np.float32)
        r = oracle_mod.project_features(maps[None], s.occ[None].astype(np.int64), s.c2w.reshape(-1), s.intr[None], s.opts(), s.grid_origin,
                                        s.voxel_size, count, out)
        assert r["rc"] == 0
        ref, ref_count = int_reference(r["hits"], maps, n_rows)
        _cache[name] = (s, maps, r["hits"], count, out, ref, ref_count)
    return _cache[name]


def test_maps_are_small_integers_with_the_pixel_code():
    m = exact_maps(3, 5, 7, 9, seed=1)
    assert m.dtype == np.float32 and m.shape == (3, 5, 7, 9)
    assert np.array_equal(m, np.rint(m)) and np.abs(m).max() <= 1023 and not np.signbit(m[m == 0]).any()
    v, y, x = np.meshgrid(np.arange(3), np.arange(5), np.arange(7), indexing="ij")
    assert (m[..., 0] == 1).all() and np.array_equal(m[..., 1], x) and np.array_equal(m[..., 2], y) and np.array_equal(m[..., 3], v + 1)
    assert np.abs(m[..., 4:]).max() <= 64 and len(np.unique(m[..., 4:])) > 50
    few = exact_maps(3, 5, 7, 3, seed=1)                        # below four channels: no code, random integers only
    assert np.abs(few).max() <= 64 and len(np.unique(few[..., 0])) > 20
    assert np.array_equal(exact_maps(3, 5, 7, 9, seed=1), m) and not np.array_equal(exact_maps(3, 5, 7, 9, seed=2), m)
    big = exact_maps(1, 416, 640, 4, seed=1)
    assert big[..., 1].max() == 639 and big[..., 2].max() == 415


@pytest.mark.parametrize("C", [3, 8, 520])
def test_fp16_maps_are_the_same_numbers(C):
    m32, m16 = exact_maps(4, 32, 48, C, seed=5), exact_maps(4, 32, 48, C, seed=5, dtype=np.float16)
    assert m16.dtype == np.float16
    assert m16.astype(np.float32).tobytes() == m32.tobytes()


@pytest.mark.parametrize("name", list(SCENES))
def test_the_oracle_leaves_the_integer_reference(oracle_mod, name):
    s, maps, hits, count, out, ref, ref_count = _case(oracle_mod, name)
    assert np.array_equal(count, ref_count)
    assert_headroom(ref_count, maps)
    assert out.tobytes() == ref.astype(np.float32).tobytes()
    assert_exact(out, ref, ref_count, name)
    if maps.shape[-1] >= 4:
        assert np.array_equal(ref[:, 0], ref_count)              # channel 0 is the constant 1
    assert not ref[0].any() and ref_count[0] == 0
    largest = {"six_views": 468, "nine_views": 479, "one_large_view": 10108}[name]
    assert int(ref_count.max()) == largest, int(ref_count.max())
    if name == "six_views":
        assert int((ref_count > 64).sum()) == 9
    if name == "one_large_view":
        assert int((hits > 0).sum()) == 266203


def _serial(rows):
    acc = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        acc = acc + r                                            # float32 + float32, one pixel after the other
    assert acc.dtype == np.float32
    return acc


def test_every_order_of_the_largest_row_leaves_the_same_bytes(oracle_mod):
    s, maps, hits, count, out, ref, ref_count = _case(oracle_mod, "one_large_view")
    row = int(ref_count.argmax())
    rows = maps.reshape(-1, maps.shape[-1])[hits.reshape(-1) == row]             # (v, y, x) order
    assert len(rows) == 10108 and rows.dtype == np.float32
    want = ref[row].astype(np.float32).tobytes()
    assert np.abs(ref[row]).max() > 2 ** 21                     # large sums: most float32 bits of the x column are in use
    assert _serial(rows).tobytes() == want
    assert _serial(rows[::-1]).tobytes() == want
    assert _serial(rows[np.random.default_rng(3).permutation(len(rows))]).tobytes() == want
    for px in (5, 32, 65):
        parts = [_serial(rows[k:k + px]) for k in range(0, len(rows), px)]
        assert len(parts) == -(-len(rows) // px)
        assert _serial(np.stack(parts)).tobytes() == want, px   # the parts' rows added in slot order
    # a map scaled by 2^15 is refused: its sums no longer fit 24 bits
    with pytest.raises(AssertionError, match="no headroom"):
        assert_headroom(ref_count, maps * np.float32(2 ** 15))


def test_headroom_is_judged_from_counts_and_values():
    maps = exact_maps(2, 8, 8, 8, seed=1)
    assert_headroom(np.array([0, 100, 2 ** 24 // 64 - 1]), maps)
    with pytest.raises(AssertionError, match="no headroom"):
        assert_headroom(np.array([0, 100, 2 ** 24 // 64]), maps)
    with pytest.raises(AssertionError, match="no headroom"):
        assert_headroom(np.array([0, 600]), maps * np.float32(2 ** 15))


def _pixel_of(hits, row, k):
    """The k-th pixel (v, y, x) of ``row`` in (v, y, x) order."""
    v, y, x = np.nonzero(hits[0] == row)
    return int(v[k]), int(y[k]), int(x[k])


def test_assert_exact_names_a_lost_and_a_doubled_pixel(oracle_mod):
    s, maps, hits, count, out, ref, ref_count = _case(oracle_mod, "six_views")
    split = ref_count > 64
    row = int(np.nonzero(split)[0][3])
    v, y, x = _pixel_of(hits, row, 17)
    assert (v, y, x) != (0, 0, 0)
    assert_exact(ref.astype(np.float32), ref, ref_count, "clean", split=split)
    for sign, word in ((-1, "lacks"), (+1, "holds twice")):
        got = ref.astype(np.float32)
        got[row] += np.float32(sign) * maps[v, y, x]
        with pytest.raises(AssertionError) as e:
            assert_exact(got, ref, ref_count, "mutated", split=split)
        msg = str(e.value)
        assert f"row {row}: {int(ref_count[row])} pixels, split=True" in msg, msg
        assert f"the row {word} pixel (v, y, x) = ({v}, {y}, {x})" in msg, msg
        assert "mutated: 1 of 2001 rows differ" in msg and f"channels 0..3 = [{sign}, {sign * x}, {sign * y}, {sign * (v + 1)}]" in msg, msg
    # a one-wavefront row, no split flags given, and a difference that is no single pixel
    light = int(np.nonzero((ref_count > 0) & ~split)[0][5])
    got = ref.astype(np.float32)
    got[light, 5] += 3
    got[row, :4] += np.float32(2) * maps[v, y, x][:4]
    with pytest.raises(AssertionError) as e:
        assert_exact(got, ref, ref_count, "two rows")
    msg = str(e.value)
    assert "two rows: 2 of 2001 rows differ" in msg and "pixel (v, y, x)" not in msg, msg
    assert f"row {light}: {int(ref_count[light])} pixels, split=n/a, got - ref of channels 0..3 = [0, 0, 0, 0], 1 of 12 channels differ" in msg, msg
    assert f"row {row}: " in msg and "4 of 12 channels differ" in msg, msg


def test_assert_exact_sees_what_a_tolerance_would_not(oracle_mod):
    """One unit in the last place of one element of a ten-thousand-pixel row, a negative zero, and rows without the pixel code."""
    s, maps, hits, count, out, ref, ref_count = _case(oracle_mod, "one_large_view")
    row = int(ref_count.argmax())
    got = ref.astype(np.float32)
    got[row, 1] = np.nextafter(got[row, 1], np.float32(np.inf))
    with pytest.raises(AssertionError, match=f"row {row}: 10108 pixels"):
        assert_exact(got, ref, ref_count, "ulp")
    got = ref.astype(np.float32)
    empty = int(np.nonzero(ref_count == 0)[0][1])
    got[empty, 2] = np.float32(-0.0)
    with pytest.raises(AssertionError, match=f"row {empty}: 0 pixels"):
        assert_exact(got, ref, ref_count, "negative zero")
    few = exact_maps(1, 416, 640, 3, seed=9)
    ref3, cnt3 = int_reference(hits, few, len(ref_count))
    got = ref3.astype(np.float32)
    got[row, 2] -= 1
    with pytest.raises(AssertionError, match=r"channels 0..2 = \[0, 0, -1\], 1 of 3 channels differ"):
        assert_exact(got, ref3, cnt3, "no code channels")
