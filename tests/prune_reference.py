"""numpy restatement of the pruning stage (examples/prune_mesh_after_finetuning.py:323-373 of the reference): per view a
scatter-max of the samples' compositing weights over their triangles, a running maximum over the views, the strict
``> threshold`` mask, the face selection (vertices kept) and the two per-view counts."""
import numpy as np


def view_scatter_max(weights, index_tri, n_faces):
    """float32 [n_faces]: the maximum weight of a view's samples on every triangle, 0 where none lands (the view's
    ``scatter_max`` into zeros)."""
    out = np.zeros((n_faces,), dtype=np.float32)
    np.maximum.at(out, np.asarray(index_tri, dtype=np.int64), np.asarray(weights, dtype=np.float32))
    return out


def triangle_weights(views, n_faces):
    """Running maximum over ``views`` = [(weights [S], index_tri [S]), ...]."""
    tw = np.zeros((n_faces,), dtype=np.float32)
    for weights, index_tri in views:
        tw = np.maximum(tw, view_scatter_max(weights, index_tri, n_faces))
    return tw


def sample_counts(views, valid_threshold=1e-3):
    """(num_samples, num_valid_samples) int64 [n_views]: ``len(weights)`` and ``sum(weights > valid_threshold)``."""
    thr = np.float32(valid_threshold)
    return (np.array([len(w) for w, _ in views], dtype=np.int64),
            np.array([int((np.asarray(w, dtype=np.float32) > thr).sum()) for w, _ in views], dtype=np.int64))


def keep_mask(tw, threshold=1e-3):
    return np.asarray(tw, dtype=np.float32) > np.float32(threshold)


def prune(vertices, faces, views, threshold=1e-3, valid_threshold=1e-3):
    """(triangle weights, mask, vertices unchanged, kept faces in order, num_samples, num_valid_samples)."""
    faces = np.asarray(faces)
    tw = triangle_weights(views, faces.shape[0])
    mask = keep_mask(tw, threshold)
    ns, nv = sample_counts(views, valid_threshold)
    return tw, mask, np.asarray(vertices), faces[mask], ns, nv
