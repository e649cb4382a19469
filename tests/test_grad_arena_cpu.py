"""Host logic of grad_arena.py on CPU tensors: the queue of work deferred to the end of a backward pass, its one way in
(ArenaState.queue_*), and what flush_deferred hands to the C ABI.  The ABI `call` and the stream lookup are replaced by a
recorder; the passes are real autograd backward passes, so the end-of-pass callback is the engine's own."""
import ctypes

import pytest
import torch

STREAM = 77
X3 = 2          # _capi.PREC_BF16X3


def _snap(a):
    if isinstance(a, ctypes.Array):
        if issubclass(a._type_, ctypes.Structure):
            return [{f: getattr(e, f) for f, _ in e._fields_} for e in a]
        return list(a)
    return a


class Arena:
    """five CPU parameters registered with one ArenaState over a flat gradient buffer; `log` records ABI calls and readiness"""

    def __init__(self, pkg, monkeypatch):
        self.ga = ga = pkg.grad_arena
        self.log = []
        self.flushes = 0
        monkeypatch.setattr(ga, "call", lambda name, *args: self.log.append((name,) + tuple(_snap(a) for a in args)))
        monkeypatch.setattr(ga, "_stream", lambda: STREAM)
        real_flush = ga.flush_deferred

        def counted(st=None):
            self.flushes += 1
            real_flush(st)
        monkeypatch.setattr(ga, "flush_deferred", counted)
        self.params = [torch.nn.Parameter(torch.zeros(s)) for s in [(8, 16), (16, 8), (8,), (12, 8), (4,)]]
        self.offs, n = [], 0
        for p in self.params:
            self.offs.append(n)
            n += (p.numel() + 7) // 8 * 8
        self.grad = torch.zeros(n)
        self.views = [self.grad[o:o + p.numel()].view_as(p) for p, o in zip(self.params, self.offs)]
        self.st = ga.register_grad_sinks(zip(self.params, self.views), ga.ArenaState())
        self.st.ready_cb.append(lambda p: self.log.append(("ready", p)))

    def names(self):
        return [e[0] for e in self.log]


@pytest.fixture()
def arena(pkg, monkeypatch):
    a = Arena(pkg, monkeypatch)
    yield a
    a.ga.clear_grad_sinks(a.st)


def backward_pass(body):
    """one real backward pass whose only node runs `body`"""
    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            body()
            return g
    Node.apply(torch.zeros(1, requires_grad=True)).sum().backward()


def bf16(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


@pytest.mark.parametrize("kind", ["wgrad", "wgrad_bf16", "colsum", "reduce"])
def test_every_queue_method_arms_one_callback_per_pass(arena, kind):
    st, v = arena.st, arena.views
    dy, x, part = torch.zeros(8, 8), torch.zeros(8, 16), torch.zeros(3 * 8)
    entry = {"wgrad": lambda: st.queue_wgrad(dy, x, v[0], 0), "wgrad_bf16": lambda: st.queue_wgrad_bf16(bf16(8, 8), bf16(8, 16), v[0]),
             "colsum": lambda: st.queue_colsum(dy, v[2], 8, 8, 8), "reduce": lambda: st.queue_reduce(part, v[2], 8, 3)}[kind]
    entered = {"wgrad": "unetr_gemm_grouped_wgrad", "wgrad_bf16": "unetr_gemm_bf16_grouped_wgrad", "colsum": "unetr_colsum_grouped",
               "reduce": "unetr_reduce_rows_grouped"}[kind]

    def body():
        entry()
        assert st.deferred.armed and arena.flushes == before and not arena.log        # armed by the method itself, launched later
        entry()
        st.queue_colsum(dy, v[4], 8, 4, 8)
    for n_pass in (1, 2):                        # the second pass arms again: the flush disarmed the queue
        before = arena.flushes
        arena.log.clear()
        backward_pass(body)
        assert arena.flushes == n_pass and not st.deferred.armed
        assert arena.names().count(entered) == 1 and arena.log[arena.names().index(entered)][2] == (3 if kind == "colsum" else 2)


def test_flush_order_and_problem_fields(arena):
    st, v, p = arena.st, arena.views, arena.params
    H = 4
    dyb, xb = bf16(8, 8), bf16(8, 16)                  # -> v[0] [8, 16]
    dyb2, xb2 = bf16(16, 16), bf16(16, 8)              # -> v[1] [16, 8]
    dy3, x3 = torch.zeros(8, 8), torch.zeros(8, 16)    # bf16x3, aligned
    dy4, x4 = torch.zeros(8, 12), torch.zeros(8, 8)    # bf16x3, N = 12: not a multiple of 8 -> generic launch
    o3, o4 = torch.zeros(8, 16), torch.zeros(12, 8)
    part_ln = torch.zeros(2 * 2 * H)                   # LayerNorm partials [nblk = 2, 2H]
    rows_bf = bf16(8, 8)
    part_r = torch.zeros(5 * 27)
    fuse = dict(index={v[0].data_ptr(): 0}, done=[], wt_done=[], arena=arena.ga._capi.AdamWArena(), flat=dict(shadow_t=bf16(4)))
    st.fuse = fuse
    ret = []

    def body():        # queued in the reverse of the launch order
        st.queue_colsum(part_ln, v[4], 2, H, 2 * H)
        st.queue_colsum(part_ln[H:], v[2][:H], 2, H, 2 * H)
        st.queue_colsum(rows_bf, v[2], 8, 8, 8)
        st.queue_wgrad(dy4, x4, o4, X3)
        st.queue_wgrad(dy3, x3, o3, X3)
        st.queue_wgrad_bf16(dyb2, xb2, v[1])
        st.queue_wgrad_bf16(dyb, xb, v[0])
        st.queue_reduce(part_r, v[3], 27, 5)
        ret.append(arena.ga._ret(p[4], v[4]))                        # complete now
        ret.append(arena.ga._ret(p[0], v[0], deferred=True))         # complete after the launches
    backward_pass(body)
    st.fuse = None
    assert ret == [None, None] and p[4].grad is v[4] and p[0].grad is v[0]
    assert arena.names() == ["ready", "unetr_reduce_rows_grouped", "unetr_gemm_bf16_grouped_wgrad_adamw_t", "unetr_gemm_bf16_grouped_wgrad",
                             "unetr_split_stack_bf16_grouped", "unetr_gemm_bf16_grouped_wgrad", "unetr_gemm_grouped_wgrad",
                             "unetr_colsum_grouped", "ready"]
    ready0, red, fused, plain, split, stack, generic, colsum, ready1 = arena.log
    assert ready0[1] is p[4] and ready1[1] is p[0]
    assert red[1:] == ([dict(part=part_r.data_ptr(), dst=v[3].data_ptr(), n=27, rows=5)], 1, STREAM)
    # only the destination named by fuse["index"] rides on the AdamW launch; its index comes back in fuse["done"] / ["wt_done"]
    assert fused[1] == [dict(dy=dyb.data_ptr(), x=xb.data_ptr(), dw=v[0].data_ptr(), M=8, N=8, K=16)] and fused[2] == 1
    assert fused[3]._obj is fuse["arena"] and fused[4] == [0] and fused[5:] == (fuse["flat"]["shadow_t"].data_ptr(), STREAM)
    assert fuse["done"] == [0] and fuse["wt_done"] == [0]
    assert plain[1:] == ([dict(dy=dyb2.data_ptr(), x=xb2.data_ptr(), dw=v[1].data_ptr(), M=16, N=16, K=8)], 1, STREAM)
    # the aligned bf16x3 entry: two split problems into 3M-row stacks, then the bf16 launch over the stacks
    s0, s1 = split[1]
    assert split[2:] == (2, STREAM)
    assert (s0["src"], s0["rows"], s0["cols"], s0["second"]) == (dy3.data_ptr(), 8, 8, 0)
    assert (s1["src"], s1["rows"], s1["cols"], s1["second"]) == (x3.data_ptr(), 8, 16, 1)
    assert stack[1:] == ([dict(dy=s0["dst"], x=s1["dst"], dw=o3.data_ptr(), M=24, N=8, K=16)], 1, STREAM)
    assert generic[1:] == ([dict(dy=dy4.data_ptr(), x=x4.data_ptr(), dw=o4.data_ptr(), M=8, N=12, K=8)], 1, X3, STREAM)
    assert colsum[1:] == ([dict(x=part_ln.data_ptr(), out=v[4].data_ptr(), ld=2 * H, M=2, N=H, x_bf16=0),
                           dict(x=part_ln.data_ptr() + 4 * H, out=v[2].data_ptr(), ld=2 * H, M=2, N=H, x_bf16=0),
                           dict(x=rows_bf.data_ptr(), out=v[2].data_ptr(), ld=8, M=8, N=8, x_bf16=1)], 3, STREAM)


def test_fused_launch_without_twins_and_bf16_communication_form(arena, monkeypatch):
    st, v = arena.st, arena.views
    q = [(bf16(8, 8), bf16(8, 16), v[0]), (bf16(16, 16), bf16(16, 8), v[1])]
    index = {v[1].data_ptr(): 1, v[0].data_ptr(): 0}
    # UNETR_AMD_WT=0 is read when the pass is flushed: no twin pointer, nothing reported as written
    fuse = dict(index=index, done=[], wt_done=[], arena=arena.ga._capi.AdamWArena(), flat=dict(shadow_t=bf16(4)))
    st.fuse = fuse
    monkeypatch.setenv("UNETR_AMD_WT", "0")
    backward_pass(lambda: [st.queue_wgrad_bf16(*e) for e in q])
    (name, probs, n, _, idx, wt, stream), = arena.log
    assert name == "unetr_gemm_bf16_grouped_wgrad_adamw_t" and n == 2 and idx == [0, 1] and wt is None and stream == STREAM
    assert [e["dw"] for e in probs] == [v[0].data_ptr(), v[1].data_ptr()]
    assert fuse["done"] == [0, 1] and fuse["wt_done"] == []
    # the data-parallel step's bf16 communication epilogue takes its own entry point
    arena.log.clear()
    comm = dict(kind="bf16out", index={v[1].data_ptr(): 1}, done=[], grad=1024, out=2048, total=arena.grad.numel())
    st.fuse = comm
    backward_pass(lambda: [st.queue_wgrad_bf16(*e) for e in q])
    st.fuse = None
    assert arena.names() == ["unetr_gemm_bf16_grouped_wgrad_bf16out", "unetr_gemm_bf16_grouped_wgrad"]
    out, plain = arena.log
    assert [e["dw"] for e in out[1]] == [v[1].data_ptr()] and out[2:] == (1, 1024, 2048, arena.grad.numel(), STREAM)
    assert [e["dw"] for e in plain[1]] == [v[0].data_ptr()] and comm["done"] == [1]


def test_mixed_precision_in_one_flush_raises(arena):
    st, v = arena.st, arena.views

    def body():
        st.queue_wgrad(torch.zeros(8, 8), torch.zeros(8, 16), v[0], 0)
        st.queue_wgrad(torch.zeros(8, 16), torch.zeros(8, 8), v[1], X3)
    with pytest.raises(RuntimeError, match="precision"):
        backward_pass(body)
    assert not arena.log and not st.deferred.armed and not st.deferred.wgrad


def test_reset_deferred_drops_the_pass(arena):
    st, v, p = arena.st, arena.views, arena.params
    x = torch.zeros(8, 8)

    def failed():
        st.queue_colsum(x, v[2], 8, 8, 8)
        st.queue_reduce(x, v[4], 4, 2)
        arena.ga._ret(p[2], v[2], deferred=True)
        st.reset_deferred()
    backward_pass(failed)
    d = st.deferred
    assert not arena.log and not d.armed and not (d.reduce or d.wgrad_bf16 or d.wgrad or d.colsum or d.params)
    backward_pass(lambda: st.queue_colsum(x, v[2], 8, 8, 8))               # the next pass arms and launches on its own
    assert arena.names() == ["unetr_colsum_grouped"] and arena.log[0][2] == 1


def test_destinations(arena, pkg):
    ga, st, v, p = arena.ga, arena.st, arena.views, arena.params
    assert ga.dest(p[0])[0] is st and ga.dest(p[0])[1] is v[0]
    assert pkg.functional._gout(p[1]) is v[1]
    assert ga.dest(torch.zeros(3)) == (None, None)
    got, (g0, g2) = ga.dests(p[0], p[2])
    assert got is st and g0 is v[0] and g2 is v[2]
    p[2].grad = torch.zeros(8)                     # a parameter that already carries .grad accumulates outside the arena
    assert ga.dest(p[2]) == (None, None) and pkg.functional._gout(p[2]) is None
    got, (g0, g2) = ga.dests(p[0], p[2])
    assert got is None and g0 is v[0] and g2 is None
    other = torch.nn.Parameter(torch.zeros(4))
    st2 = ga.register_grad_sinks([(other, torch.zeros(4))], ga.ArenaState())
    try:
        assert ga.dest(other)[0] is st2 and ga.dests(p[0], other)[0] is None      # two owners: nothing is queued together
    finally:
        ga.clear_grad_sinks(st2)
    assert ga.dest(other) == (None, None) and ga.dest(p[0])[0] is st
