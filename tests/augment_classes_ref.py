"""CPU restatements of class-balanced crop sampling (a helper module, not a test file), built on augment_ref.

MONAI is not a dependency of this project.  Each MONAI 0.6.0 fact below is restated from memory of that release and says so
in a "MONAI 0.6.0:" comment; the tests pin the HIP kernels (csrc/augment.hip) to these restatements.

(i)  class_index_lists_ref: VolumeCache.build_class_indices, map_classes_to_indices in numpy.
(ii) pick_class, draw_row_classes, replay_classes: the sampler's params table and class record of sampling="label_classes"
     replayed bit for bit.  Block 0 of a sample changes meaning (word 0 the class, word 1 the voxel); every other word is
     augment_ref.draw_row's.
"""
import math

import numpy as np
import torch

import augment_ref as R


# ---------------------------------------------------------------- (i) the lists
def class_index_lists_ref(label, image, num_classes, image_mask=False, thr=0.0):
    # MONAI 0.6.0 map_classes_to_indices(label, num_classes, image, image_threshold):
    #   img_flat = np.any(image > image_threshold, axis=0).ravel()                (only with an image)
    #   channels = label.shape[0]; if channels == 1 and num_classes is None: raise ValueError
    #   for c in range(num_classes if channels == 1 else channels):
    #       label_flat = np.any(label[c : c + 1] if channels > 1 else label == c, axis=0).ravel()
    #       label_flat = np.logical_and(img_flat, label_flat) if img_flat is not None else label_flat
    #       indices.append(np.nonzero(label_flat)[0])
    label, image = np.asarray(label), np.asarray(image)
    L = label.shape[0]
    if L == 1 and num_classes is None:
        raise ValueError("num_classes is required for a single-channel label")
    if L > 1 and num_classes not in (None, L):
        raise ValueError("num_classes must be None or the number of label channels")
    mask = np.any(image > thr, axis=0).ravel() if image_mask else None
    out = []
    for c in range(num_classes if L == 1 else L):
        flat = (label[c] != 0).ravel() if L > 1 else (label[0] == c).ravel()
        if mask is not None:
            flat = np.logical_and(mask, flat)
        out.append(np.nonzero(flat)[0])
    return out


# ---------------------------------------------------------------- (ii) the draws
def pick_class(ratios, counts, u):
    # MONAI 0.6.0 generate_label_classes_crop_centers(spatial_size, num_samples, label_spatial_shape, indices, ratios, rand_state):
    #   ratios_ = [1] * len(indices) if ratios is None else ratios; a negative ratio raises
    #   for i, array in enumerate(indices): if len(array) == 0: warn, ratios_[i] = 0
    #   classes = rand_state.choice(len(ratios_), size=num_samples, p=np.asarray(ratios_) / np.sum(ratios_))
    #   per sample: indices_to_use = indices[classes[i]]; random_int = rand_state.randint(len(indices_to_use)); unravel_index
    #   then correct_crop_centers.
    # choice(p=...) is a search of u in the cumulative sums; here: the first c with u * total < cum_c, sums in class order in
    # double over the float32 ratios, the last class of positive weight if rounding falls through.  A ratio that is negative or
    # not finite (possible only in a device tensor nobody checked) counts as 0.  None: no class has weight.
    eff = []
    for r, n in zip(ratios, counts):
        r = float(np.float32(r))
        eff.append(r if n > 0 and r > 0.0 and math.isfinite(r) else 0.0)
    total, last = 0.0, None
    for c, e in enumerate(eff):
        total += e
        if e > 0.0:
            last = c
    if last is None:
        return None
    t, cum = u * total, 0.0
    for c, e in enumerate(eff):
        cum += e
        if e > 0.0 and t < cum:
            return c
    return last


def draw_row_classes(cfg, seed, call, s, vol, shape, lists, ratios):
    """(params row, class) of sample s on volume `vol` of spatial shape `shape` with per-class index lists `lists`; class -1 and
    a uniform corner from words 0..2 when no class has weight"""
    b0 = R.sample_words(seed, call, s)[0]
    S = cfg["spatial_size"]
    row = R.draw_row({**cfg, "sampling": "uniform"}, seed, call, s, vol, shape, (), ())      # blocks 1, 2 and the uniform corner
    cls = pick_class(ratios, [len(a) for a in lists], R.u01(b0[0]))
    if cls is None:
        return row, -1
    idx = int(lists[cls][R.randint(b0[1], len(lists[cls]))])
    center = list(np.unravel_index(idx, shape))
    row[1:4] = R.crop_corner(R.correct_crop_centers(center, S, shape), S)
    return row, cls


def replay_classes(cfg, volumes, ratios, order, ncalls, call=0, cursor=0):
    """(params tables, class records) of `ncalls` calls; volumes: list of (spatial shape, per-class lists).  The schedule is
    augment_ref.replay's."""
    B, ns = cfg["batch_size"], cfg["num_samples"]
    tables, classes = [], []
    for _ in range(ncalls):
        rows, cl = [], []
        for s in range(B):
            vol = int(order[(cursor + s // ns) % len(order)])
            shape, lists = volumes[vol]
            row, c = draw_row_classes(cfg, cfg["seed"], call, s, vol, shape, lists, ratios)
            rows.append(row)
            cl.append(c)
        tables.append(torch.tensor(rows, dtype=torch.int32))
        classes.append(torch.tensor(cl, dtype=torch.int32))
        call += 1
        cursor = (cursor + B // ns) % len(order)
    return tables, classes
