"""Generates tests/golden/cluster_golden.npz and tests/golden/README_cluster.md with the tool the reference's clustering
scripts use (script/debug_checks_scripts/voxel_cluster_to_ply.py and three more): the scripts' own expression,

    KMeans(n_clusters=10, random_state=0, n_init=10).fit_predict(rows)

on label_sums_reference.planted_scene(6000, 32, 10, 0.5, SCENE) -- once on the unit-normalised rows, whose partition is stored
(and asserted to be the planted one), and once on the raw rows as the scripts feed them, whose adjusted Rand index against
the planted labels goes into the README: the reason cluster_features.py does not copy the reference's metric.
Stored: labels int16 [6000], the scene's parameters and a checksum of its rows (the tests rebuild the scene from the seed).
Usage: python tests/golden/make_cluster_golden.py"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import label_sums_reference as ref  # noqa: E402

SCENE = dict(N=6000, C=32, K=10, sigma=0.5, seed=1)


def scene():
    return ref.planted_scene(SCENE["N"], SCENE["C"], SCENE["K"], SCENE["sigma"], SCENE["seed"])


def checksum(rows):
    return hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest()


def main():
    from sklearn.cluster import KMeans
    rows, truth, _ = scene()
    x = rows.astype(np.float64)
    unit = x / np.linalg.norm(x, axis=1, keepdims=True)
    on_unit = KMeans(n_clusters=10, random_state=0, n_init=10).fit_predict(unit)
    on_raw = KMeans(n_clusters=10, random_state=0, n_init=10).fit_predict(x)
    ari_unit, ari_raw = ref.adjusted_rand(on_unit, truth), ref.adjusted_rand(on_raw, truth)
    assert ref.same_partition(on_unit, truth) and ari_unit == 1.0, "KMeans on the unit rows did not find the planted partition"
    np.savez(os.path.join(HERE, "cluster_golden.npz"), labels=on_unit.astype(np.int16), rows_sha256=np.array(checksum(rows)),
             **{f"scene_{k}": np.array(v) for k, v in SCENE.items()})
    with open(os.path.join(HERE, "README_cluster.md"), "w") as f:
        f.write("# cluster_golden.npz\n\n"
                "Written by `make_cluster_golden.py` with scikit-learn's `KMeans(n_clusters=10, random_state=0, n_init=10)`, the\n"
                "expression of the reference's clustering scripts, on `planted_scene(6000, 32, 10, 0.5, 1)` of\n"
                "`tests/label_sums_reference.py` (10 planted directions, row norms drawn from [0.5, 4]).\n\n"
                "| rows given to KMeans | adjusted Rand index against the planted labels |\n|---|---|\n"
                f"| unit-normalised (stored in `labels`) | {ari_unit:.2f} |\n"
                f"| raw, as the reference scripts feed them | {ari_raw:.2f} |\n\n"
                "The Euclidean metric on rows whose norms vary splits and merges the planted directions; on unit rows it is the\n"
                "cosine metric up to a monotone map and finds them all.  `cluster_features.py` therefore clusters by cosine, and\n"
                "`tests/test_gpu_cluster_cli.py` holds its partition to the stored one up to a renaming of the ids.\n")
    print(f"unit rows: ARI {ari_unit:.4f}; raw rows: ARI {ari_raw:.4f}")


if __name__ == "__main__":
    main()
