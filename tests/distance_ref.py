"""References for the distance transform, the distance fields and the two distance-map losses (csrc/edt.hip, csrc/dist_loss.hip), and
the builders of the inputs their tests share.  Everything here is float64 / int64 torch on the CPU; nothing calls the package.

  edt_ref              brute force: the minimum over all (non-zero voxel, zero voxel) pairs, chunked; int64 squared steps without a
                       spacing, float64 from the float32-rounded spacing otherwise; +inf for a mask without a zero
  field_ref            the signed / unsigned field of one binary object from two edt_ref calls
  boundary_loss_ref    } plain differentiable torch: autograd gives the reference gradient
  hausdorff_dt_loss_ref
  make_mask            the mask kinds of the transform's tests
  loss_inputs          seeded logits and targets of a loss case, the logits moved out of the threshold band (below)
"""
import math

import torch

SPACING = (3.0, 0.7, 1.5)
BAND = 1e-3
_CACHE = {}


def _coords(idx, shape):
    z = idx // (shape[1] * shape[2])
    y = (idx // shape[2]) % shape[1]
    x = idx % shape[2]
    return torch.stack([z, y, x], 1)


def edt_ref(mask, spacing=None, squared=False):
    """mask [D,H,W] (anything `!= 0` makes a bool of) -> the distance of every voxel to the nearest voxel where mask == 0.
    Without a spacing and squared: int64, exact.  Results are cached by content and never modified by the callers."""
    m = (torch.as_tensor(mask) != 0).contiguous()
    shape = tuple(m.shape)
    key = (m.numpy().tobytes(), shape, spacing, squared)
    if key in _CACHE:
        return _CACHE[key]
    flat = m.reshape(-1)
    q = _coords(flat.nonzero().flatten(), shape)          # the voxels that have a distance to find
    zc = _coords((~flat).nonzero().flatten(), shape)      # all candidates
    exact = spacing is None
    if exact:
        out = torch.zeros(flat.numel(), dtype=torch.int64)
    else:
        out = torch.zeros(flat.numel(), dtype=torch.float64)
        s = torch.tensor(spacing, dtype=torch.float32).double()          # the voxel sizes the kernel is given
    if q.shape[0]:
        if zc.shape[0] == 0:
            out = torch.full((flat.numel(),), math.inf, dtype=torch.float64)
        else:
            best = []
            chunk = max(1, (1 << 21) // zc.shape[0])
            qa = q if exact else q.double() * s          # (positions in mm: the products are exact in float64)
            za = zc if exact else zc.double() * s
            for i in range(0, q.shape[0], chunk):
                d2 = None
                for a in range(3):
                    d = qa[i:i + chunk, a, None] - za[None, :, a]
                    d2 = d * d if d2 is None else d2.addcmul_(d, d)
                best.append(d2.min(1).values)
            out[flat] = torch.cat(best)
    out = out.reshape(shape)
    if not squared:
        out = out.double().sqrt()
    _CACHE[key] = out
    return out


def field_ref(obj, spacing=None, unsigned=False):
    """obj [D,H,W] bool -> float64 field: signed = d_fg outside, -(d_bg - u) inside, u = 1 or the smallest spacing; unsigned =
    d_fg + d_bg; 0 everywhere for an object that is empty or fills the volume"""
    obj = torch.as_tensor(obj) != 0
    if not obj.any() or obj.all():
        return torch.zeros(obj.shape, dtype=torch.float64)
    d_bg, d_fg = edt_ref(obj, spacing), edt_ref(~obj, spacing)
    if unsigned:
        return d_fg + d_bg
    u = 1.0 if spacing is None else float(torch.tensor(min(spacing), dtype=torch.float32))
    return torch.where(obj, -(d_bg - u), d_fg)


def fields_ref(objs, spacing=None, unsigned=False):
    """[B,C,D,H,W] -> the field of every (b, c) object"""
    return torch.stack([torch.stack([field_ref(o, spacing, unsigned) for o in item]) for item in objs])


def _probs_and_target(z, target, multilabel):
    if multilabel:
        return torch.sigmoid(z), target.double()
    C = z.shape[1]
    g = torch.zeros(z.shape, dtype=torch.float64)
    g.scatter_(1, target.long(), 1.0)
    assert g.shape[1] == C
    return torch.softmax(z, 1), g


def boundary_loss_ref(z, target, multilabel=False, include_background=False, spacing=None, weight=1.0):
    """z float64 [B,C,*S] (requires_grad for the gradient); target class ids [B,1,*S] or a mask [B,C,*S]"""
    p, g = _probs_and_target(z, target, multilabel)
    phi = fields_ref(g != 0, spacing)
    c0 = 0 if include_background else 1
    return weight * (p[:, c0:] * phi[:, c0:]).mean()


def hausdorff_dt_loss_ref(z, target, multilabel=False, include_background=False, spacing=None, weight=1.0, alpha=2.0):
    p, g = _probs_and_target(z, target, multilabel)
    f_g = fields_ref(g != 0, spacing, unsigned=True)
    f_p = fields_ref(p.detach() > 0.5, spacing, unsigned=True)
    c0 = 0 if include_background else 1
    return weight * (((p - g) ** 2) * (f_p ** alpha + f_g ** alpha))[:, c0:].mean()


# ---------------------------------------------------------------------------------------------- inputs of the transform's tests
# (D, H, W).  The first eight: the smallest volume; a 64-lane boundary on one axis with extents of 1 on the others; non-cubic (an axis
# mix-up); an odd cube; one past a 32-column tile and a 64-row boundary; a line longer than two waves; a mid-size cube.  Then one
# shape on each side of every tile parameter of csrc/edt.hip:
#   64 x per mask word (x pass):            (2, 3, 64) | (1, 2, 65)          4 x-lines per block (x pass):     (2, 2, 130) | (1, 5, 3)
#   EDT_COLS = 32 columns per tile:         (2, 3, 32) | (3, 70, 33)         8 rows per sweep (256 / 32):      (8, 9, 5): n = 8 and 9
#   EDT_TALL = 256 (two fields, z pass):    (256, 2, 3) | (257, 2, 3)        EDT_COLS_TALL = 16 beyond it:     (257, 1, 16) | (257, 1, 17)
#   the extent cap 512 (64 KiB of LDS):     (512, 2, 2), (2, 512, 2), (1, 2, 512)
EDT_SHAPES = [(1, 1, 1), (1, 1, 70), (70, 1, 1), (5, 7, 9), (17, 17, 17), (3, 70, 33), (2, 2, 130), (24, 24, 24),
              (2, 3, 64), (1, 2, 65), (1, 5, 3), (2, 3, 32), (8, 9, 5), (256, 2, 3), (257, 2, 3), (257, 1, 16), (257, 1, 17),
              (512, 2, 2), (2, 512, 2), (1, 2, 512)]
MASK_KINDS = ("random", "three_zeros", "corner_zero", "all_zeros", "no_zeros", "half_space", "hollow_sphere")


def make_mask(kind, shape, seed=0):
    """bool [D,H,W], True = non-zero"""
    gen = torch.Generator().manual_seed(seed + 7919 * MASK_KINDS.index(kind) + sum(shape))
    V = shape[0] * shape[1] * shape[2]
    if kind == "random":
        return torch.rand(shape, generator=gen) < 0.5
    m = torch.ones(shape, dtype=torch.bool)
    if kind == "three_zeros":
        m.view(-1)[torch.randperm(V, generator=gen)[:3]] = False
    elif kind == "corner_zero":
        m[-1, -1, -1] = False
    elif kind == "all_zeros":
        m[:] = False
    elif kind == "half_space":
        ax = max(range(3), key=lambda a: shape[a])
        idx = [slice(None)] * 3
        idx[ax] = slice(0, shape[ax] // 2)
        m[tuple(idx)] = False
    elif kind == "hollow_sphere":
        g = torch.meshgrid(*[(torch.arange(n, dtype=torch.float64) + 0.5) / n - 0.5 for n in shape], indexing="ij")
        r = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2).sqrt()
        m = (r >= 0.2) & (r < 0.4)
    return m


# -------------------------------------------------------------------------------------------------- inputs of the losses' tests
def band_count(logits, multilabel):
    p = torch.sigmoid(logits.double()) if multilabel else torch.softmax(logits.double(), 1)
    return int(((p - 0.5).abs() < BAND).sum())


def out_of_band(logits, multilabel):
    """The Hausdorff-DT loss thresholds p at 0.5; a probability within BAND of it could fall on either side in float32 and in
    float64.  Every float32 logit whose float64 probability lies in the band gets 0.5 added, until none is left (under the softmax
    only the first such channel of a voxel: with two channels both are in the band together, and raising both changes nothing)."""
    z = logits.clone()
    for _ in range(64):
        p = torch.sigmoid(z.double()) if multilabel else torch.softmax(z.double(), 1)
        hit = (p - 0.5).abs() < BAND
        if not hit.any():
            break
        if not multilabel:
            hit &= hit.cumsum(1) == 1
        z[hit] += 0.5
    assert band_count(z, multilabel) == 0
    return z


def _blob_objects(C, S, gen):
    """[C,S,S,S] bool: a centred sphere, a half-space, then spheres elsewhere"""
    ax = torch.arange(S, dtype=torch.float64)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    objs = []
    for c in range(C):
        if c % 3 == 0:
            ctr = (S - 1) / 2 + (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * (2.0 if c else 0.0)
            objs.append(((zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2).sqrt() < 0.42 * S)
        elif c % 3 == 1:
            objs.append([zz, yy, xx][(c // 3) % 3] >= S - max(2, S // 4) - c // 3)
        else:
            ctr = torch.rand(3, generator=gen, dtype=torch.float64) * (S - 1)
            objs.append(((zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2).sqrt() < 0.22 * S)
    return torch.stack(objs)


_INPUTS = {}


def loss_inputs(shape, mode, label="noise", logit="randn"):
    """(logits float32 out of the band, target float32) of a case; CPU, shared, never modified.
    mode "oh": class ids [B,1,S,S,S]; "ml": mask [B,C,S,S,S].  label "noise": as the segmentation losses' tests draw them; "blob":
    spheres and half-spaces; "degenerate": class 1 absent from item 0 (and the last item one class only, when B > 1).
    logit "randn": 2 * randn; "prior": a shifted copy of the target's objects (+-3) plus randn."""
    key = (shape, mode, label, logit)
    if key in _INPUTS:
        return _INPUTS[key]
    B, C, S = shape
    gen = torch.Generator().manual_seed(1000 * C + S)
    noise = torch.randn(B, C, S, S, S, generator=gen)
    if label == "blob":
        objs = torch.stack([_blob_objects(C if mode == "ml" else C - 1, S, gen) for _ in range(B)])
        if mode == "ml":
            t = objs.float()
        else:
            t = torch.zeros(B, 1, S, S, S)
            for c in range(C - 1):
                t[:, 0][objs[:, c]] = float(c + 1)
    elif mode == "ml":
        t = (torch.rand(B, C, S, S, S, generator=gen) < 0.35).float()
        if label == "degenerate":
            t[0, 0] = 0
            t[-1, -1] = 1
    else:
        t = torch.randint(0, C, (B, 1, S, S, S), generator=gen).float()
        if label == "degenerate":
            t[0][t[0] == 1] = 0.0
            if B > 1:
                t[-1] = float(C - 1)
    if logit == "prior":
        g = t if mode == "ml" else torch.zeros(B, C, S, S, S).scatter_(1, t.long(), 1.0)
        logits = 3.0 * (2.0 * torch.roll(g, shifts=(1, -2), dims=(2, 4)) - 1.0) + noise
    else:
        logits = noise * 2
    _INPUTS[key] = (out_of_band(logits, mode == "ml"), t, band_count(logits, mode == "ml"))
    return _INPUTS[key]


ONEHOT = dict(to_onehot_y=True, softmax=True)
MULTI = dict(to_onehot_y=False, sigmoid=True)
A, B4, C3, D14, E1 = (1, 2, 17), (2, 4, 16), (2, 3, 24), (1, 14, 12), (1, 1, 17)
SP = SPACING

# (id, loss, shape, mode, label, logit, options): every shape in both forms, (1, 1, 17) multilabel only; each of include_background,
# spacing, alpha and weight in both of its values under both losses and both forms
LOSS_CASES = [
    ("bl-oh-A", "boundary", A, "oh", "noise", "randn", dict()),
    ("bl-oh-A-bg-sp-w", "boundary", A, "oh", "blob", "prior", dict(include_background=True, spacing=SP, weight=0.37)),
    ("bl-ml-A-bg", "boundary", A, "ml", "noise", "randn", dict(include_background=True)),
    ("bl-oh-B4-sp", "boundary", B4, "oh", "noise", "prior", dict(spacing=SP)),
    ("bl-ml-B4-w", "boundary", B4, "ml", "blob", "randn", dict(weight=0.37)),
    ("bl-oh-C3-blob", "boundary", C3, "oh", "blob", "prior", dict(weight=0.37)),
    ("bl-ml-C3-sp", "boundary", C3, "ml", "noise", "randn", dict(spacing=SP, include_background=True)),
    ("bl-oh-D14", "boundary", D14, "oh", "noise", "randn", dict(include_background=True)),
    ("bl-ml-D14-blob", "boundary", D14, "ml", "blob", "prior", dict()),
    ("bl-ml-E1", "boundary", E1, "ml", "noise", "randn", dict(include_background=True, weight=0.37)),
    ("bl-oh-B4-degenerate", "boundary", B4, "oh", "degenerate", "randn", dict(include_background=True)),
    ("hd-oh-A-a1", "hausdorff", A, "oh", "noise", "randn", dict(alpha=1.0)),
    ("hd-oh-A-blob-bg-sp", "hausdorff", A, "oh", "blob", "prior", dict(include_background=True, spacing=SP)),
    ("hd-ml-A-w", "hausdorff", A, "ml", "blob", "randn", dict(weight=0.37)),
    ("hd-oh-B4-w-bg", "hausdorff", B4, "oh", "noise", "randn", dict(weight=0.37, include_background=True)),
    ("hd-ml-B4-a1-sp", "hausdorff", B4, "ml", "noise", "prior", dict(alpha=1.0, spacing=SP)),
    ("hd-oh-C3-blob", "hausdorff", C3, "oh", "blob", "prior", dict()),
    ("hd-ml-C3-bg", "hausdorff", C3, "ml", "noise", "randn", dict(include_background=True)),
    ("hd-oh-D14-sp", "hausdorff", D14, "oh", "blob", "randn", dict(spacing=SP, alpha=1.0, weight=0.37)),
    ("hd-ml-D14", "hausdorff", D14, "ml", "noise", "prior", dict(include_background=True)),
    ("hd-ml-E1-blob", "hausdorff", E1, "ml", "blob", "prior", dict(include_background=True, alpha=1.0)),
    ("hd-oh-B4-degenerate", "hausdorff", B4, "oh", "degenerate", "randn", dict()),
]


def loss_ref(loss, z, target, mode, opts):
    fn = boundary_loss_ref if loss == "boundary" else hausdorff_dt_loss_ref
    return fn(z, target, multilabel=mode == "ml", **opts)
