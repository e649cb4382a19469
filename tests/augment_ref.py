"""CPU restatements of the GPU-resident training augmentation (a helper module, not a test file).

MONAI is not a dependency of this project.  Each MONAI 0.6.0 fact below is restated from memory of that release and says so
in a "MONAI 0.6.0:" comment; the tests pin the HIP kernels (csrc/augment.hip) to these restatements.

(i)   philox4x64_10 and the word-to-draw assignment: the sampler's params table replayed bit for bit (replay).
(ii)  correct_crop_centers, the pos/neg and uniform crop corners.
(iii) source_index: the composed index map the gather implements; augment_seq: the same as sequential torch.flip / torch.rot90.
(iv)  scale_ref, foreground_box_ref, index_lists_ref: VolumeCache.add; apply_ref: a whole batch from a params table.
"""
import math
import struct

import numpy as np
import torch

M64 = (1 << 64) - 1
PARAM_COLS = 8


# ---------------------------------------------------------------- (i) Philox4x64-10 and the draws
def philox4x64_10(ctr, key):
    """Philox4x64-10 (Salmon et al., SC'11), the generator of numpy.random.Philox: 10 rounds, key bumped before rounds 2..10.
    numpy.random.Philox(key=k, counter=c).random_raw(4) == philox4x64_10(c + 1, k): numpy increments its counter before each
    block (tests/test_augment_cpu.py pins this convention)."""
    c, k = [int(v) & M64 for v in ctr], [int(v) & M64 for v in key]
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B97F4A7C15) & M64, (k[1] + 0xBB67AE8584CAA73B) & M64]
        p0, p1 = 0xD2E7470EE14C6C93 * c[0], 0xCA5A826395121157 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k[0], p1 & M64, (p0 >> 64) ^ c[3] ^ k[1], p0 & M64]
    return c


def u01(w):
    """uniform double in [0, 1) from one 64-bit word: (w >> 11) * 2**-53 (numpy's next_double)"""
    return (w >> 11) * 2.0 ** -53


def randint(w, n):
    """integer in [0, n) from one 64-bit word: (w * n) >> 64"""
    return (w * n) >> 64


def sample_words(seed, call, s):
    """the 12 words of sample s in call `call`: block j has counter (call, s, j, 0) and key (seed, 0).
    Assignment:  block 0: pos_neg -> [0] u < pos_ratio picks the list, [1] randint(len(list));  uniform -> [0..2] corner per axis
                 block 1: [0..2] u < flip_prob[a] flips spatial axis a, [3] u < rot90_prob rotates
                 block 2: [0] k = randint(max_k) + 1, [1] u < shift_prob shifts, [2] offset = lo + (hi - lo) * u"""
    return [philox4x64_10((call, s, j, 0), (seed, 0)) for j in range(3)]


# ---------------------------------------------------------------- (ii) crop centres
def correct_crop_centers(centers, spatial_size, label_spatial_shape):
    # MONAI 0.6.0 (monai.transforms.utils.correct_crop_centers):
    #   valid_start = np.floor_divide(spatial_size, 2)
    #   valid_end = np.subtract(label_spatial_shape + np.array(1), spatial_size / np.array(2)).astype(np.uint16)
    #   if valid_start[i] == valid_end[i]: valid_end[i] += 1   (np.random.randint needs start < end)
    #   centre < valid_start -> valid_start; centre >= valid_end -> valid_end - 1
    out = []
    for c, s, d in zip(centers, spatial_size, label_spatial_shape):
        vs = s // 2
        ve = int(math.floor(d + 1 - s / 2))
        if vs == ve:
            ve += 1
        if c < vs:
            c = vs
        if c >= ve:
            c = ve - 1
        out.append(int(c))
    return out


def crop_corner(center, spatial_size):
    # MONAI 0.6.0 SpatialCrop(roi_center, roi_size): roi_start = max(center - floor_divide(roi_size, 2), 0)
    return [max(c - s // 2, 0) for c, s in zip(center, spatial_size)]


def draw_row(cfg, seed, call, s, vol, shape, fg, bg):
    """one params row (vol, z0, y0, x0, flip mask, k, shift flag, offset float bits) of sample s, volume `vol` of spatial
    shape `shape` with index lists fg / bg (sequences of ints)"""
    b0, b1, b2 = sample_words(seed, call, s)
    S = cfg["spatial_size"]
    if cfg["sampling"] == "pos_neg":
        # MONAI 0.6.0 generate_pos_neg_label_crop_centers: an empty list forces pos_ratio to 0 (no fg) or 1 (no bg); per sample
        # `fg if R.rand() < pos_ratio else bg`, then R.randint(len(list)), np.unravel_index, correct_crop_centers
        pr = 0.0 if len(fg) == 0 else (1.0 if len(bg) == 0 else cfg["pos_ratio"])
        lst = fg if u01(b0[0]) < pr else bg
        idx = int(lst[randint(b0[1], len(lst))])
        center = list(np.unravel_index(idx, shape))
        corner = crop_corner(correct_crop_centers(center, S, shape), S)
    else:
        # MONAI 0.6.0 RandSpatialCrop(random_size=False) / get_random_patch: corner R.randint(0, dim - size + 1) per axis
        corner = [randint(b0[a], shape[a] - S[a] + 1) for a in range(3)]
    flips = sum(1 << a for a in range(3) if u01(b1[a]) < cfg["flip_prob"][a])
    # MONAI 0.6.0 RandRotate90: k = R.randint(max_k) + 1, applied with probability prob
    k = randint(b2[0], cfg["max_k"]) + 1 if u01(b1[3]) < cfg["rot90_prob"] else 0
    # MONAI 0.6.0 RandShiftIntensity: offset = R.uniform(low, high) = low + (high - low) * R.random(); img + offset in float32
    shift = int(u01(b2[1]) < cfg["shift_prob"])
    lo, hi = cfg["shift_range"]
    off = float(np.float32(lo + (hi - lo) * u01(b2[2]))) if shift else 0.0
    bits = struct.unpack("<i", struct.pack("<f", off))[0]
    return [vol, *corner, flips, k, shift, bits]


def aug_config(aug):
    return dict(spatial_size=aug.spatial_size, sampling=aug.sampling, pos_ratio=aug.pos_ratio, flip_prob=aug.flip_prob,
                rot90_prob=aug.rot90_prob, max_k=aug.max_k, shift_prob=aug.shift_prob, shift_range=aug.shift_range,
                num_samples=aug.num_samples, batch_size=aug.batch_size, seed=aug.seed)


def replay(cfg, volumes, order, ncalls, call=0, cursor=0):
    """params tables of `ncalls` calls starting at device call counter `call` and cursor `cursor`; volumes: list of
    (spatial shape, fg list, bg list).  Item i of a call takes order[(cursor + i) % len(order)], samples item-major."""
    B, ns = cfg["batch_size"], cfg["num_samples"]
    tables = []
    for _ in range(ncalls):
        rows = []
        for s in range(B):
            vol = int(order[(cursor + s // ns) % len(order)])
            shape, fg, bg = volumes[vol]
            rows.append(draw_row(cfg, cfg["seed"], call, s, vol, shape, fg, bg))
        tables.append(torch.tensor(rows, dtype=torch.int32))
        call += 1
        cursor = (cursor + B // ns) % len(order)
    return tables


# ---------------------------------------------------------------- (iii) the composed index map
def source_index(S, corner, flips, k, axes=(0, 1)):
    """for every output voxel of a crop of size S (3-tuple): its source coordinates in the volume, as the gather maps them
    (int64 [3, S0, S1, S2]): undo np.rot90(k, axes), then the flips, then add the corner"""
    o = torch.stack(torch.meshgrid(*[torch.arange(s) for s in S], indexing="ij"))
    p = o.clone()
    a, b = axes
    n = S[a]
    k %= 4
    if k == 1:
        p[a], p[b] = o[b], n - 1 - o[a]
    elif k == 2:
        p[a], p[b] = n - 1 - o[a], n - 1 - o[b]
    elif k == 3:
        p[a], p[b] = n - 1 - o[b], o[a]
    for ax in range(3):
        if flips >> ax & 1:
            p[ax] = S[ax] - 1 - p[ax]
    return p + torch.tensor(corner).view(3, 1, 1, 1)


def augment_seq(vol, corner, S, flips, k, axes=(0, 1)):
    """vol [C, D, H, W]: crop, RandFlipd per axis (np.flip), then RandRotate90d (MONAI 0.6.0: np.rot90(img, k, (a+1, b+1)) on
    channel-first arrays; torch.rot90 has the same convention)"""
    z, y, x = corner
    out = vol[:, z:z + S[0], y:y + S[1], x:x + S[2]]
    for ax in range(3):
        if flips >> ax & 1:
            out = torch.flip(out, dims=(ax + 1,))
    if k % 4:
        out = torch.rot90(out, k, dims=(axes[0] + 1, axes[1] + 1))
    return out


# ---------------------------------------------------------------- (iv) add() and a whole batch
def scale_ref(img, a_min, a_max, b_min, b_max):
    # MONAI 0.6.0 ScaleIntensityRange(clip=True) on float32 arrays, Python scalars cast to float32:
    #   if a_max - a_min == 0.0: return img - a_min
    #   img = (img - a_min) / (a_max - a_min); img = img * (b_max - b_min) + b_min; np.clip(img, b_min, b_max)
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    img = img.float()
    if a_max - a_min == 0.0:
        return img - f(a_min)
    img = (img - f(a_min)) / f(a_max - a_min)
    img = img * f(b_max - b_min) + f(b_min)
    return torch.minimum(torch.maximum(img, f(b_min)), f(b_max))


def foreground_box_ref(img):
    # MONAI 0.6.0 CropForegroundd(source_key="image", select_fn=x > 0, margin=0): box of np.any(select_fn(img), axis=0),
    # end exclusive; returns (start, end) or None when no voxel is selected
    m = (img > 0).any(0)
    if not bool(m.any()):
        return None
    idx = m.nonzero()
    return idx.min(0).values.tolist(), (idx.max(0).values + 1).tolist()


def index_lists_ref(label, img, image_threshold=0.0):
    # MONAI 0.6.0 map_binary_to_indices(label, image, image_threshold):
    #   label_flat = np.any(label, axis=0).ravel(); fg = np.nonzero(label_flat)[0]
    #   img_flat = np.any(image > image_threshold, axis=0).ravel(); bg = np.nonzero(img_flat & ~label_flat)[0]
    lab = (label != 0).any(0).reshape(-1)
    im = (img > image_threshold).any(0).reshape(-1)
    return lab.nonzero().view(-1), (im & ~lab).nonzero().view(-1)


def normalize_ref(x):
    """NormalizeIntensityd(nonzero=True, channel_wise=True) of one sample x [C, ...] (float32): per channel over x != 0,
    mean and population std in float64 cast to float32, std 0 -> 1, nothing to do without nonzero voxels.
    MONAI 0.6.0 _normalize: slices = img != 0; if not np.any(slices): return img; _sub = np.mean(img[slices]);
    _div = np.std(img[slices]); if _div == 0.0: _div = 1.0; img[slices] = (img[slices] - _sub) / _div"""
    x = x.clone()
    for c in range(x.shape[0]):
        m = x[c] != 0
        if not bool(m.any()):
            continue
        v = x[c][m].double()
        mean = v.mean()
        sd = float(np.float32(float(((v * v).mean() - mean * mean).clamp_min(0).sqrt())))
        sd = 1.0 if sd == 0.0 else sd
        x[c][m] = (x[c][m] - torch.tensor(float(mean), dtype=torch.float32)) / torch.tensor(sd, dtype=torch.float32)
    return x


def apply_ref(images, labels, params, S, axes=(0, 1), normalize=False):
    """x [B, C, *S], y [B, L, *S] (float32) from a params table; images / labels: per volume [C,D,H,W] float32 / [L,D,H,W]"""
    xs, ys = [], []
    for r in params.tolist():
        vol, corner, flips, k, shift, bits = r[0], r[1:4], r[4], r[5], r[6], r[7]
        x = augment_seq(images[vol], corner, S, flips, k, axes).clone()
        y = augment_seq(labels[vol], corner, S, flips, k, axes).float()
        if shift:
            x = x + torch.tensor(struct.unpack("<f", struct.pack("<i", bits))[0], dtype=torch.float32)
        if normalize:
            x = normalize_ref(x)
        xs.append(x)
        ys.append(y)
    return torch.stack(xs), torch.stack(ys)
