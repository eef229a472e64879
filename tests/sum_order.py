"""A numpy twin of the two-step float64 sum every loss family ends in (csrc/vp_reduce.h), operation for operation:

  step 1  tree_sum     a workgroup's ``threads`` slots, zeros where a thread has no element, added by a halving tree:
                       slot t += slot t + h for h = threads / 2, .., 1; the total is slot 0.
  step 2  ordered      the workgroups' totals added one by one in ascending index, starting from 0.0.

Float64 addition is correctly rounded in numpy as on the device, so the twin applied to the float32 terms a call returns
gives the bits of the call's statistic -- as long as the order is the contract's.  tests/test_sum_order_cpu.py checks the twin
itself, tests/test_gpu_sum_order.py the device against it."""
import numpy as np


def tree_sum(values, threads):
    """The halving tree over the last axis of ``values`` (at most ``threads`` slots, a power of two; missing slots are
    zeros), in float64.  Leading axes are independent workgroups: the result has their shape."""
    v = np.asarray(values, np.float64)
    assert threads & (threads - 1) == 0 and v.shape[-1] <= threads
    s = np.zeros(v.shape[:-1] + (threads,), np.float64)
    s[..., :v.shape[-1]] = v
    h = threads // 2
    while h >= 1:
        s[..., :h] = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def ordered(partials):
    """The partials added left to right in float64, starting from 0.0: a sequential loop, never a pairwise np.sum."""
    a = np.float64(0.0)
    for p in np.asarray(partials, np.float64).reshape(-1):
        a = a + p
    return a


def tile_slots(image, tile):
    """A [H,W] map cut into tile x tile workgroups in row-major tile order: [tiles, tile * tile] with pixel (tx, ty) of a tile
    in slot tile * ty + tx and zeros outside the image."""
    image = np.asarray(image)
    H, W = image.shape
    ty, tx = -(-H // tile), -(-W // tile)
    p = np.zeros((ty * tile, tx * tile), image.dtype)
    p[:H, :W] = image
    return p.reshape(ty, tile, tx, tile).transpose(0, 2, 1, 3).reshape(ty * tx, tile * tile)


def chunk_slots(values, threads):
    """A flat array cut into consecutive workgroups of ``threads`` elements: [workgroups, threads], zeros past the end."""
    values = np.asarray(values).reshape(-1)
    n = -(-len(values) // threads)
    p = np.zeros(n * threads, values.dtype)
    p[:len(values)] = values
    return p.reshape(n, threads)


def two_step(slots, threads):
    """tree_sum of every workgroup of ``slots`` [workgroups, <= threads], then ordered over the workgroups."""
    return ordered(tree_sum(slots, threads))


def ascending(values):
    """The plain left-to-right float64 sum of the elements in storage order: what the contract's order is compared with."""
    return ordered(values)


def bits(x):
    return np.float64(x).tobytes()
