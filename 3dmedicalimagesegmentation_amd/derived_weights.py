"""Copies derived from the fp32 master weights: bf16 shadows, bf16x3 words, transposed bf16 twins, packed conv weights (DESIGN section 4
has the table of their rules).  Every copy is one `Derived` record in the table of its kind, trusted through `in_step` and `readable`.
functional.py imports this module and fills in `_stream`; nothing here imports functional.  `call`, `_stream`, `_capturing` and
`_pack_bytes` are the only doors to the device and the library (tests/test_derived_weights_cpu.py replaces them).
"""
import os
import weakref

import torch

from . import _capi, grad_arena
from ._capi import call

_stream = None        # hook set by functional.py: () -> id of the current stream


def _capturing():
    """the only place that asks (the query raises on a machine without a device)"""
    return torch.cuda.is_current_stream_capturing()


def _pack_bytes(w, kind, prec):
    """size of the packed form `kind` of conv weight `w`"""
    if kind == 4:          # transposed conv [in, out, 2, 2, 2] -> bf16 [in][tap][out]
        return w.numel() * 2
    cin, cout = (w.shape[0], w.shape[1]) if kind == 3 else (w.shape[1], w.shape[0])      # (kind 3: the 1x1x1 conv transposed)
    lib = _capi.load()
    return lib.unetr_conv3_packed_bytes(cin, cout, kind, prec) if kind <= 1 else lib.unetr_conv3_packed_1x1_bytes(cin, cout, prec)


# A copy that no optimizer of this package keeps in step is trusted for ONE "weight epoch": every forward pass (begin_forward) and
# every write behind torch's back that this package makes or is told of (invalidate_weight_shadows) starts a new one.
_EPOCH = [0]


class _Kind:
    """One kind of derived copy: its tables, its getter (Derived.get) and whether an unmaintained copy of it is bound to the weight
    epoch.  Words and twins are not: they stay valid until torch touches the parameter or invalidate_weight_shadows() says so."""
    def __init__(self, name, epoch_bound):
        self.name, self.epoch_bound, self.get = name, epoch_bound, None
        self.table = {}        # id(p) -> record; packs: (id(p), kind, prec).  Keys are reused after a parameter dies: lookups validate
        self.by_addr = {}      # bf16, twins: the same records by storage address (functional._prefetch is handed detached aliases)


BF16, WORDS, TWIN, PACK = _Kind("bf16", True), _Kind("x3", False), _Kind("twin", False), _Kind("pack", True)


class Derived:
    """one derived copy of one parameter"""
    __slots__ = ("kind", "buf", "param", "version", "addr", "epoch", "maintained", "arena", "offset", "padded", "pack")

    def __init__(self, kind, buf, w, version=-1, addr=0, epoch=-1, maintained=False, arena=None, offset=0, padded=0, pack=()):
        self.kind, self.buf, self.param = kind, buf, weakref.ref(w)       # (id(p) keys are reused after a parameter dies)
        # version and address of the parameter and the weight epoch at the last derive; maintained: an optimizer of this package rewrites buf
        self.version, self.addr, self.epoch, self.maintained = version, addr, epoch, maintained
        # twin: its arena and the element offset in the arenas; words: elements of the padded arena slot; pack: (kind, prec)
        self.arena, self.offset, self.padded, self.pack = arena, offset, padded, pack

    def in_step(self, w, alias=False, version=True):
        """Alive, `w` itself (alias: or a detached alias of it, which shares storage and version counter), same version (version=False:
        whatever the version), same address (a re-pointed parameter -- `p.data = other` -- keeps its version counter)."""
        p = self.param()
        return p is not None and (alias or p is w) and (not version or self.version == w._version) and self.addr == w.data_ptr()

    def readable(self, capturing=None):
        """may be read without re-deriving (given in_step): maintained, or derived in this epoch and not under capture"""
        return (self.maintained or not self.kind.epoch_bound
                or (self.epoch == _EPOCH[0] and not (_capturing() if capturing is None else capturing)))

    def stamp(self, w):
        self.version, self.addr, self.epoch = w._version, w.data_ptr(), _EPOCH[0]

    def read_as_is(self):
        """would a capture starting now READ this copy as it is (instead of re-deriving it inside the graph)?  (SlidingWindowInferer)"""
        return self.in_step(self.param()) and self.readable(capturing=True)

    def get(self):
        return self.kind.get(self.param(), *self.pack)

    def current(self):
        """the record now registered where this one was (a getter replaces the record when the buffer has to change), or None"""
        p = self.param()
        return self.kind.table.get((id(p),) + self.pack if self.pack else id(p)) if p is not None else None


def records_of(params):
    """the bf16 shadows, words and packs registered for the living parameters `params` (twins are not read by a forward pass)"""
    params = {id(p): p for p in params}
    out = []
    for pid, p in params.items():
        out += [rec for rec in (BF16.table.get(pid), WORDS.table.get(pid)) if rec is not None and rec.param() is p]
    return out + [rec for key, rec in PACK.table.items() if key[0] in params and rec.param() is params[key[0]]]


def invalidate_weight_shadows():
    """Declare every derived weight copy (bf16 shadows, packed conv weights) stale.  MANDATORY after writing a parameter
    through ``.data`` in place (``p.data.copy_()``, ``p.data.mul_()``, an EMA swap, a hand-written broadcast) once the
    copies are optimizer-maintained (this package's AdamW has stepped): such a write changes neither the version counter
    nor the storage address, so nothing else can notice it.  Everything torch can see is handled automatically: in-place
    ops on the parameter, torch optimizers, ``load_state_dict``, re-pointed ``.data``, and -- for copies no optimizer of
    this package maintains -- any change at all between two forward passes (``begin_forward``).

    Captured inference graphs (inference.SlidingWindowInferer) follow the same contract.  A forward captured under no_grad
    reads derived copies in two ways: a copy that no optimizer of this package maintained at capture time is re-derived INSIDE
    the graph (weight_bf16 / conv_pack_get never trust an epoch under capture), so every replay is current; a copy that was
    optimizer-maintained at capture time -- and the bf16x3 word shadow -- is read as it is.  Before the first replay of every
    call the inferer therefore starts a new weight epoch and walks the as-is copies through these same getters eagerly: nothing
    happens to a copy that is still maintained and in step, a stale one (version counter, address, or this function) is
    re-derived into the same buffer, which the graph then reads.  If a parameter, a derived buffer or the scratch workspace has
    moved since capture, the graph is captured again.  A live TrainStep on the same model needs nothing extra: its optimizer
    kernels rewrite the buffers the inference graph reads."""
    _EPOCH[0] += 1
    for kind in (BF16, WORDS, TWIN, PACK):
        for rec in kind.table.values():
            rec.version = -1


def refresh_derived_weights(model):
    """Re-derive, eagerly and into the SAME buffers, every derived weight copy of ``model`` (bf16 shadows, bf16x3 words, transposed
    twins, packed conv weights) that is out of step with its parameter.  A captured TrainStep reads the copies its optimizer kernels
    maintain as they are -- a replay runs no Python that could notice a change -- so this is the call to make after
    ``model.load_state_dict()`` (or any other write torch can see) on a model whose training step is ALREADY captured: resuming
    from a checkpoint after capture.  Copies that are current are left alone; before capture nothing is needed (the first forward
    re-derives on demand).  ``.data`` writes behind the version counter still need invalidate_weight_shadows() first."""
    if _capturing():
        raise RuntimeError("refresh_derived_weights launches derive kernels: not while a hipGraph is being captured")
    for rec in records_of(model.parameters()):          # bf16 and words per parameter, then the packs
        rec.get()
    flat = getattr(model, "_flat", None)
    if flat is not None and flat.get("shadow_t") is not None:       # the twins, from the bf16 shadow arena made current above
        _wt_derive(flat, _stale_twins(flat))


def begin_forward():
    """a new pass starts a new weight epoch: the first use of a copy nobody maintains re-derives it (see invalidate_weight_shadows)"""
    if not _capturing():
        _EPOCH[0] += 1


# ---- bf16 shadows (bf16 precision mode: unetr_gemm_bf16 reads bf16-STORED weights) ----------------------------------------
def register_weight_shadow(w, shadow):
    """flat-arena mode: `shadow` is the bf16 view the optimizer kernel keeps in step with `w`"""
    BF16.table[id(w)] = BF16.by_addr[w.data_ptr()] = Derived(BF16, shadow, w, w._version, w.data_ptr(), _EPOCH[0], True)   # caller has just cast it


def weight_bf16(w):
    rec = BF16.table.get(id(w))
    if rec is None or rec.param() is not w or rec.buf.shape != w.shape or rec.buf.device != w.device:
        rec = Derived(BF16, torch.empty(w.shape, dtype=torch.bfloat16, device=w.device), w)
        BF16.table[id(w)] = BF16.by_addr[w.data_ptr()] = rec
    if not (rec.in_step(w) and rec.readable()):
        src = w.detach().contiguous()
        call("unetr_cast_bf16", src.data_ptr(), rec.buf.data_ptr(), src.numel(), _stream())
        # re-derived here = somebody other than this package's optimizer changed the weight (or may have): the copy is no
        # longer optimizer-maintained until that optimizer steps again (shadow_ptr_for_update / mark_flat_maintained)
        rec.stamp(w)
        rec.maintained = False
        st = grad_arena.owner(w)
        if st is not None:
            st.unmaintained += 1
    return rec.buf


def shadow_at(w):
    """the bf16 shadow of the parameter at the storage address of `w` (a detached alias), stale or not, or None; launches nothing"""
    rec = BF16.by_addr.get(w.data_ptr())
    p = rec.param() if rec is not None else None
    ok = p is not None and p.data_ptr() == w.data_ptr() and rec.buf.shape == w.shape and rec.buf.device == w.device
    return rec.buf if ok else None


def shadow_ptr_for_update(w):
    """optimizer side: where the bf16 copy of `w` lives, if the GEMMs have asked for one; the caller's kernel rewrites
    it together with the fp32 master, which makes the shadow optimizer-maintained from here on"""
    rec = BF16.table.get(id(w))
    if rec is None or not rec.in_step(w):
        return None
    rec.maintained = True
    return rec.buf.data_ptr()


def mark_flat_maintained(params, state=None):
    """flat-arena AdamW has just rewritten the whole bf16 shadow arena together with the masters: every registered shadow
    of these parameters is in step again.  Only walks the table after something of THIS model had to be re-derived: the
    count lives in the model's ArenaState (a process-wide one let model A's step clear what model B still had to redo)."""
    if state is None and params:
        state = grad_arena.owner(params[0])
    if state is not None and not state.unmaintained:
        return
    for w in params:
        rec = BF16.table.get(id(w))
        if rec is not None and rec.in_step(w, version=False):
            rec.version, rec.maintained = w._version, True
    if state is not None:
        state.unmaintained = 0


# ---- bf16x3 mode: word shadow of the weights ---------------------------------------------------------------------------------
# With flat arenas the weights' (hi, lo) split is kept as an arena of words [hi | lo << 16]: created on first use, never under capture.
def _split_words(src, dst, n):
    call("unetr_split_words", src.data_ptr(), dst.data_ptr(), n, _stream())


def weight_x3(w):
    """the weight as split words (int32 view, same shape) when `w` lives in a flat arena; else None (the kernel splits the fp32 weight)"""
    if os.environ.get("UNETR_AMD_X3_WORDS", "1") == "0":      # (A/B hook: the GEMMs split the fp32 weights in registers like the activations)
        return None
    st = grad_arena.owner(w)
    flat = st.flat if st is not None else None
    if flat is None:
        return None
    if flat.get("shadow_x3") is None:
        if _capturing():
            return None                      # (the arena must not come out of a graph's private pool)
        arena = torch.empty(flat["total"], dtype=torch.int32, device=w.device)
        _split_words(flat["param"], arena, flat["total"])
        flat["shadow_x3"] = arena
        for p, o in zip(flat["params"], flat["offsets"]):
            WORDS.table[id(p)] = Derived(WORDS, arena[o:o + p.numel()].view_as(p), p, p._version, p.data_ptr(), padded=(p.numel() + 7) // 8 * 8)
    rec = WORDS.table.get(id(w))
    if rec is None or not rec.in_step(w, version=False) or rec.buf.device != w.device:
        return None
    if not rec.in_step(w):                   # torch modified the parameter since the last derive: redo this slice (whole padded slot)
        _split_words(w, rec.buf, rec.padded)
        rec.stamp(w)
    return rec.buf


def refresh_x3_shadow(flat, written=False):
    """optimizer side (flat arenas): kernels of this package have just updated the parameter arena.  written: they wrote the words too
    (AdamW arena launches take the pointer); otherwise one derive launch over the arena -- when a word shadow exists at all"""
    arena = flat.get("shadow_x3") if flat is not None else None
    if arena is None:
        return
    if not written:
        _split_words(flat["param"], arena, flat["total"])
    for p in flat["params"]:
        rec = WORDS.table.get(id(p))
        if rec is not None and rec.in_step(p, version=False):
            rec.version = p._version


# ---- bf16 mode: transposed bf16 shadow of the ViT Linear weights -------------------------------------------------------------
# With flat arenas a second bf16 arena holds W [N, K] at arena offset o as its twin [K, N] at shadow_t + o, and the data gradients
# dx = dy . W run in the forward kernel form on it.  Both forms give the same bits, so the arena is only
# created where it is written for free: by a backward pass with the fused AdamW epilogue armed, outside graph capture.
def drop_wt_shadow(flat):
    """forget the twin arena of a model and every table entry that points into it (ArenaState.clear)"""
    arena = flat.pop("shadow_t", None) if flat is not None else None
    if arena is None:
        return
    for tab in (TWIN.table, TWIN.by_addr):
        for k in [k for k, rec in tab.items() if rec.arena is arena]:
            del tab[k]


def wt_enabled():
    """UNETR_AMD_WT=0 (A/B hook): no transposed shadow, the data gradients stay on the b_kn form"""
    return os.environ.get("UNETR_AMD_WT", "1") != "0"


def _epilogue_twin_arena(flat):
    """the twin arena of a model for the fused weight-gradient + AdamW launch to write, or None"""
    return flat.get("shadow_t") if wt_enabled() and flat is not None else None


def _wt_derive(flat, recs):
    """twins `recs` from the bf16 shadow arena (which the caller knows to be current for them) in ONE grouped launch"""
    if not recs:
        return
    arr = (_capi.TransposeProblem * len(recs))()
    for a, rec in zip(arr, recs):
        a.offset, a.K, a.N = rec.offset, rec.buf.shape[0], rec.buf.shape[1]      # (the twin is [K, N]: the weight [N, K])
    call("unetr_transpose_bf16_grouped", flat["shadow"].data_ptr(), flat["shadow_t"].data_ptr(), arr, len(recs), _stream())
    for rec in recs:
        rec.stamp(rec.param())


def _stale_twins(flat, also=None):
    """every stale registered twin of the model's arena (and `also`) whose bf16 shadow, made current here, IS the arena slice the launch reads"""
    todo = []
    for rec in TWIN.table.values():
        p = rec.param()
        if (rec.arena is flat["shadow_t"] and p is not None and (rec is also or not rec.in_step(p))
                and weight_bf16(p).data_ptr() == flat["shadow"].data_ptr() + 2 * rec.offset):
            todo.append(rec)
    return todo


def keeps_twin(st):
    """this backward pass ends in the epilogue that writes the twins (the fused AdamW form, not the bf16 communication form)"""
    fz = st.fuse if st is not None else None
    return fz is not None and fz.get("kind") != "bf16out"


def weight_bf16_t(w):
    """The transposed bf16 twin [in, out] of Linear weight `w` [out, in], or None (the caller then reads weight_bf16(w) as the
    [K, N] operand).  Never launches under graph capture; creates the arena only for a backward pass whose weight-gradient launch
    will keep it current (the fused AdamW epilogue), and under capture hands a twin out only to such a pass: the optimizer part of
    any other captured step would leave it behind from the second replay on."""
    if not wt_enabled() or w.dim() != 2 or w.shape[0] % 8 or w.shape[1] % 8:
        return None
    st = grad_arena.owner(w)
    flat = st.flat if st is not None else None
    if flat is None or flat.get("shadow") is None:
        return None
    capturing = _capturing()
    keeps = keeps_twin(st)
    if capturing and not keeps:
        return None        # a replay runs no Python: a graph may read the twin only if the graph itself rewrites it every step
    if flat.get("shadow_t") is None:
        if capturing or not keeps:
            return None
        flat["shadow_t"] = torch.zeros(flat["total"], dtype=torch.bfloat16, device=w.device)
    rec = TWIN.table.get(id(w))
    if rec is None or rec.param() is not w or rec.arena is not flat["shadow_t"]:
        index = flat.get("_index")
        if index is None:
            index = flat["_index"] = {id(p): o for p, o in zip(flat["params"], flat["offsets"])}
        off = index.get(id(w))
        if off is None or flat["shadow_t"].device != w.device:
            return None
        rec = Derived(TWIN, flat["shadow_t"][off:off + w.numel()].view(w.shape[1], w.shape[0]), w, addr=w.data_ptr(),
                      arena=flat["shadow_t"], offset=off)
        TWIN.table[id(w)] = TWIN.by_addr[w.data_ptr()] = rec
    if not rec.in_step(w):
        if capturing:
            return None
        # this twin and every other registered one of the arena that is stale (after invalidate_weight_shadows: all of them) in one launch
        todo = _stale_twins(flat, also=rec)
        if not any(r is rec for r in todo):
            return None
        _wt_derive(flat, todo)
    return rec.buf


def twin_at(w):
    """likewise the twin, where a data-gradient GEMM launched now would be handed it: current, under capture only if the pass rewrites it"""
    rec = TWIN.by_addr.get(w.data_ptr())
    ok = (rec is not None and rec.in_step(w, alias=True) and rec.buf.device == w.device and rec.buf.numel() == w.numel()
          and (keeps_twin(grad_arena.owner(w)) or not _capturing()))
    return rec.buf if ok else None


def refresh_wt_shadow(flat, stepped, written=()):
    """optimizer side (flat arenas): kernels of this package have just updated the parameters `stepped` and their bf16 shadow slices.
    written: those whose twin the same kernels wrote (the fused weight-gradient epilogue): such a twin keeps its stamp, current or
    stale.  Every other registered twin of a parameter that stepped is re-derived in one grouped launch (a step being captured only
    marks them stale: weight_bf16_t gave its backward pass no twin, and the next eager or fused pass re-derives them)."""
    if flat is None or flat.get("shadow_t") is None:
        return
    written = {id(p) for p in written}
    todo = []
    for p in stepped:
        rec = TWIN.table.get(id(p))
        if rec is None or rec.arena is not flat["shadow_t"] or rec.param() is not p or id(p) in written:
            continue
        sh = BF16.table.get(id(p))
        if (sh is not None and sh.in_step(p) and sh.buf.data_ptr() == flat["shadow"].data_ptr() + 2 * rec.offset
                and not _capturing()):
            todo.append(rec)
        else:
            rec.version = -1       # (weight_bf16_t re-derives it when a backward pass asks)
    _wt_derive(flat, todo)


# ---- packed conv weights (MFMA operand layouts of csrc/conv3.hip) ------------------------------------------------------
# kind 0 / 1: 3x3x3 forward / data gradient, 2 / 3: 1x1x1 forward / transposed.  Rules as for the bf16 shadows; without the table
# the step spent ~25 five-microsecond pack launches on its critical path.
def conv_pack_get(w, kind, prec):
    rec = PACK.table.get((id(w), kind, prec))
    if rec is None or rec.param() is not w or rec.buf.device != w.device:
        rec = Derived(PACK, torch.empty(_pack_bytes(w, kind, prec), dtype=torch.uint8, device=w.device), w, pack=(kind, prec))
        PACK.table[(id(w), kind, prec)] = rec
    if not (rec.in_step(w) and rec.readable()):
        _pack_launch([(w, rec)], prec)
        rec.stamp(w)
        rec.maintained = False
    return rec.buf


def _pack_launch(items, prec):
    arr = (_capi.PackProblem * len(items))()
    for a, (w, rec) in zip(arr, items):
        a.w, a.out, a.Cin, a.Cout, a.kind = w.data_ptr(), rec.buf.data_ptr(), w.shape[1], w.shape[0], rec.pack[0]
    call("unetr_conv3_pack_grouped", arr, len(items), prec, _stream())


def refresh_conv_packs():
    """optimizer side: re-pack every registered conv weight in one launch per precision; the packs are maintained from here on"""
    by_prec = {}
    for key, rec in list(PACK.table.items()):
        w = rec.param()
        if w is None:
            del PACK.table[key]
            continue
        if not w.is_cuda or not rec.in_step(w):
            continue                                  # torch touched the parameter: conv_pack_get re-packs on demand
        by_prec.setdefault(rec.pack[1], []).append((w, rec))
        rec.maintained = True
    for prec, items in by_prec.items():
        _pack_launch(items, prec)


def after_step(flat, stepped, *, arena, twins_written=(), repack=True):
    """Kernels of this package have just stepped the parameters `stepped` of the flat model `flat`.  arena: arena launches, which
    rewrite the bf16 shadow slices and the words with the masters; False: per-tensor launches -- each took its bf16 shadow's pointer
    (shadow_ptr_for_update), none writes words.  twins_written: whose twin they wrote.  Launches: words, twins, then packs if `repack`."""
    if arena and flat.get("shadow") is not None:
        mark_flat_maintained(stepped, flat.get("state"))
    refresh_x3_shadow(flat, written=arena)
    refresh_wt_shadow(flat, stepped, twins_written)
    if repack:
        refresh_conv_packs()


BF16.get, WORDS.get, TWIN.get, PACK.get = weight_bf16, weight_x3, weight_bf16_t, conv_pack_get
grad_arena._drop_twins, grad_arena._twin_arena = drop_wt_shadow, _epilogue_twin_arena
