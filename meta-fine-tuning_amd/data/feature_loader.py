"""Reader of the feature files `save_features` writes (mirror of the reference's data/feature_loader.py).

The container is ``.npz`` with the reference's three dataset names -- ``all_feats`` [rows, D] float32, ``all_labels`` [rows] int32,
``count`` [1] -- instead of HDF5 (h5py is not a dependency of this package)."""
import numpy as np


def save_features_file(filename, feats, labels):
    """Write ``feats`` [count, D] and ``labels`` [count] as a feature file."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if feats.ndim != 2 or labels.shape != (feats.shape[0],):
        raise ValueError("feature file: feats %s and labels %s are not [count, D] and [count]" % (feats.shape, labels.shape))
    with open(filename, "wb") as f:                       # (a file object: np.savez would append '.npz' to a bare name)
        np.savez(f, all_feats=feats, all_labels=labels, count=np.asarray([feats.shape[0]], dtype=np.int64))


def init_loader(filename):
    """-> {label: [feature row, ...]} in file order.  Rows beyond ``count`` are dropped, and so are trailing all-zero rows (the
    reference's files are allocated for the largest possible count and trimmed this way when read)."""
    with np.load(filename) as f:
        count = int(np.asarray(f["count"]).reshape(-1)[0])
        feats = np.asarray(f["all_feats"])[:count]
        labels = np.asarray(f["all_labels"])[:count]
    while feats.shape[0] > 0 and not feats[-1].any():
        feats, labels = feats[:-1], labels[:-1]
    cl_data_file = {int(c): [] for c in np.unique(labels)}
    for row, c in zip(feats, labels):
        cl_data_file[int(c)].append(row)
    return cl_data_file
