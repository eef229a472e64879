"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds of the
project can be compared output for output on the same arguments (the inputs are seeded: same arguments, same inputs).

  * integer and boolean arrays are written as float64 (exact below 2**53), float16 / float32 as float32, float64 as float64;
  * at most LIMIT_BYTES in all, headers included.  When the arrays do not fit, those larger than an eighth of the limit are
    cut to the same number of rows, drawn without replacement by a generator seeded with SEED and the array's row count
    (so the sample depends on the shapes only, never on the values), written as <name>.npy together with <name>_rows.npy,
    the row indices, ascending.  The smaller arrays are written whole.
  * the rows are gathered on the arrays' own device before anything is copied to the host.

Called after the timed region, on rank 0; never inside it."""
import os

import numpy as np

LIMIT_BYTES = 64 * 10 ** 6
SEED = 0
_HEADER = 4096         # bytes budgeted per .npy header (they take 128 for shapes of a few dimensions)


def _out_dtype(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return np.float64
    if dtype.kind == "f":
        return np.float32
    return np.float64


def sample_rows(n_rows, k, seed=SEED):
    """k distinct row indices of [0, n_rows), ascending; a function of (n_rows, k, seed) alone."""
    rng = np.random.default_rng([seed, n_rows])
    return np.sort(rng.choice(n_rows, size=k, replace=False))


def _np_dtype(a):
    import torch
    if isinstance(a, torch.Tensor):
        return torch.empty((), dtype=a.dtype).numpy().dtype
    return np.asarray(a).dtype


def _to_numpy(a):
    import torch
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return np.ascontiguousarray(a, dtype=_out_dtype(a.dtype))


def _take_rows(a, rows):
    import torch
    if isinstance(a, torch.Tensor):
        return a.index_select(0, torch.from_numpy(rows).to(a.device))
    return np.asarray(a)[rows]


def plan(shapes_dtypes, limit=LIMIT_BYTES):
    """{name: (shape, dtype)} -> (rows per sampled array or None, names of the sampled arrays)."""
    size = {n: int(np.prod(s, dtype=np.int64)) * np.dtype(_out_dtype(d)).itemsize for n, (s, d) in shapes_dtypes.items()}
    if sum(size.values()) + _HEADER * len(size) <= limit:
        return None, []
    big = [n for n in size if size[n] > limit // 8 and len(shapes_dtypes[n][0]) >= 1 and shapes_dtypes[n][0][0] > 0]
    small = sum(size[n] + _HEADER for n in size if n not in big)
    per_row = sum(size[n] // shapes_dtypes[n][0][0] + 8 for n in big)      # the row itself and its index
    k = (limit - small - 2 * _HEADER * len(big)) // per_row
    if not big or k < 1:
        raise ValueError(f"--dump-outputs: the arrays {sorted(size)} do not fit {limit} bytes")
    return int(min(k, min(shapes_dtypes[n][0][0] for n in big))), big


def dump_outputs(out_dir, arrays, limit=LIMIT_BYTES, seed=SEED):
    """Write ``arrays`` ({name: torch tensor or numpy array}) to out_dir as described above; returns {file name: shape}."""
    k, big = plan({n: (tuple(a.shape), _np_dtype(a)) for n, a in arrays.items()}, limit)
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, a in arrays.items():
        if name in big:
            rows = sample_rows(a.shape[0], k, seed)
            np.save(os.path.join(out_dir, name + "_rows.npy"), rows.astype(np.float64))
            written[name + "_rows"] = [int(k)]
            a = _take_rows(a, rows)
        a = _to_numpy(a)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = list(a.shape)
    total = sum(os.path.getsize(os.path.join(out_dir, n + ".npy")) for n in written)
    assert total <= limit, f"--dump-outputs wrote {total} bytes, more than {limit}"
    return written
