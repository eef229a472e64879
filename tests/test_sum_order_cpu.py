"""The numpy twin of the fixed-order float64 sums (tests/sum_order.py) checked on its own, without a GPU: it is exact where
every order is exact, zero padding is neutral, and on inputs spread over 40 binades it gives other bits than the plain
ascending and descending sums -- the property that lets tests/test_gpu_sum_order.py notice a changed order at all."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sum_order as so  # noqa: E402


def order_visible(n, seed, binades=20):
    """n float32 terms 2^uniform(-binades, binades) times a value in [0.2, 2]: the inputs test_gpu_sum_order.py feeds."""
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(-binades, binades, n)) * rng.uniform(0.2, 2.0, n)).astype(np.float32)


@pytest.mark.parametrize("n,threads", [(1, 256), (255, 256), (257, 256), (703, 256), (1089, 1024), (3000, 1024)])
def test_exactly_summable_integers_equal_fsum(n, threads):
    v = np.random.default_rng(n).integers(-2 ** 20, 2 ** 20, n).astype(np.float32)
    got = so.two_step(so.chunk_slots(v, threads), threads)
    assert got == math.fsum(v.tolist()) and got == so.ascending(v)


def test_tile_slots_put_pixel_tx_ty_in_slot_tile_ty_plus_tx():
    img = np.arange(1, 19 * 37 + 1, dtype=np.float32).reshape(19, 37)
    s = so.tile_slots(img, 16)
    assert s.shape == (6, 256)
    assert s[0, 16 * 3 + 5] == img[3, 5] and s[2, 16 * 2 + 4] == img[2, 36] and s[2, 16 * 2 + 5] == 0
    assert s[4, 16 * 2 + 1] == img[18, 17] and s[4, 16 * 3] == 0
    assert so.two_step(s, 256) == math.fsum(img.reshape(-1).tolist())


@pytest.mark.parametrize("seed", range(5))
def test_zero_padded_tail_changes_nothing(seed):
    v = order_visible(200, seed).astype(np.float64)
    padded = np.concatenate([v, np.zeros(56)])
    assert so.bits(so.tree_sum(v, 256)) == so.bits(so.tree_sum(padded, 256))
    assert so.bits(so.tree_sum(v, 256)) == so.bits(so.tree_sum(v[None], 256)[0])
    parts = so.tree_sum(so.chunk_slots(order_visible(703, seed), 256), 256)
    assert so.bits(so.ordered(parts)) == so.bits(so.ordered(np.concatenate([parts, np.zeros(253)])))


@pytest.mark.parametrize("seed", range(20))
def test_the_order_is_visible_over_40_binades(seed):
    """The three orders never agree.  Two of them differ by a few units in the last place, so any two can still round to the
    same double: about one seed in four does that for one of the pairs (the next test names seeds where none does)."""
    v = order_visible(703, seed)
    twin = so.two_step(so.chunk_slots(v, 256), 256)
    up, down = so.ascending(v), so.ascending(v[::-1])
    assert len({so.bits(twin), so.bits(up), so.bits(down)}) >= 2
    assert abs(twin - up) <= 1e-12 * abs(up) and abs(twin - down) <= 1e-12 * abs(up)      # other bits, the same number


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("tiled", [False, True])
def test_the_twin_differs_from_the_ascending_and_the_descending_sum(seed, tiled):
    """703 terms as three workgroups of 256 slots, or as the six 16 x 16 tiles of a 37 x 19 image: other bits than both plain
    loops.  Fixed seeds: see above."""
    v = order_visible(703, seed + (21 if tiled else 0))
    slots = so.tile_slots(v.reshape(19, 37), 16) if tiled else so.chunk_slots(v, 256)
    twin = so.two_step(slots, 256)
    assert so.bits(twin) != so.bits(so.ascending(v)) and so.bits(twin) != so.bits(so.ascending(v[::-1]))


@pytest.mark.parametrize("seed", range(20))
def test_the_order_is_invisible_over_20_binades(seed):
    """Terms of similar size sum exactly in float64 whatever the order: why a comparison with a reference inside a bound, or
    of two runs with each other, cannot see the order."""
    v = order_visible(703, seed, binades=10)
    twin = so.two_step(so.chunk_slots(v, 256), 256)
    assert so.bits(twin) == so.bits(so.ascending(v)) == so.bits(so.ascending(v[::-1])) == so.bits(math.fsum(v.tolist()))
