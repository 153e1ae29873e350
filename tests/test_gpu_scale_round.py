"""GPU: the RNS scale-and-round by t/Q (include/nflhip.h "BFV multiplication", nfllib_amd/csrc/kernels_scale_round.hip), word for
word against the Python-integer restatement of tests/scale_round_util.py: no tolerance anywhere.  The shapes are the smallest at
which each path runs: both register plans, the chunked two-pass fallback, 16-byte groups and single words, a batch that wraps the
grid-stride loop.  Inputs are batches of 3 of full-range random words with the values that put the first rounding and the second
conversion on their edges and inside their bands planted in polynomials 0 and 1 (tests/test_scale_round_cpu.py planted)."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
import scale_round_util as S
from test_scale_round_cpu import planted

pytestmark = pytest.mark.gpu

N = 64
# (limb_bits, nm, ks, t, batch): the <4, 5> plan; the <8, 9> plan; the chunked first pass + k_baseconv
PLAN_A = [(64, 5, 2, 65537, 3), (64, 9, 4, 2**58 + 12345, 3), (64, 3, 1, 3, 3), (32, 5, 2, 257, 3), (32, 7, 3, 2**29 - 1, 3)]
PLAN_B = [(64, 12, 5, 65537, 3)]
FALLBACK = [(32, 36, 17, 257, 2)]
_CASES, _ENGINES = {}, {}


def case(e, ks, t, batch, n=N):
    """the input and, computed once and kept, the expected words of (floor, keep)"""
    key = (e.limb_bits, e.degree, e.nmoduli, ks, t, batch)
    if key not in _CASES:
        a = np.ascontiguousarray(planted(e.P, e.limb_bits, ks, t, n=n)[:batch]) if n >= 16 else B.random_batch(e.P, n, batch, e.np_dtype, 3)
        a.setflags(write=False)
        _CASES[key] = (a, {})
    a, wants = _CASES[key]

    def want(floor=False, keep=False):
        if (floor, keep) not in wants:
            wants[(floor, keep)] = S.scale_round_rns(a, e.P, ks, t, floor=floor, keep=keep)
        return wants[(floor, keep)]
    return a, want


def rows_engine(e, first, count):
    """the engine over rows [first, first + count) of e's moduli: the transforms of a result's layout"""
    from nfllib_amd import Engine
    key = (e.limb_bits, e.degree, first, count)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(e.limb_bits, e.degree, count, device=0, rows=list(range(first, first + count)))
    return _ENGINES[key]


def check_shape(e, ks, t, batch, n=N):
    import torch
    nm, kd = e.nmoduli, e.nmoduli - ks
    a, want = case(e, ks, t, batch, n)
    d = e.to_device(a)
    dn = e.ntt_(d.clone())
    for floor, keep in ((False, False), (True, False), (False, True), (True, True)):
        w = want(floor, keep)
        got = e.scale_round(d, ks, t, floor=floor, keep=keep)
        assert got.shape == (batch, kd if keep else ks, n)
        assert np.array_equal(e.to_host(got), w), (ks, t, floor, keep)
        two = e.scale_round(d, ks, t, floor=floor, keep=keep, plan="two_pass")
        assert torch.equal(two, got), (ks, t, floor, keep, "two_pass")
        child = rows_engine(e, ks, kd) if keep else rows_engine(e, 0, ks)
        fwd = child.ntt_(got.clone())
        for plan in (None, "two_pass"):
            assert torch.equal(e.scale_round(dn, ks, t, floor=floor, keep=keep, ntt=True, plan=plan), fwd), (ks, t, floor, keep, plan, "ntt")
    assert np.array_equal(e.h_scale_round(a, ks, t), want()) and np.array_equal(e.h_scale_round(a, ks, t, keep=True), want(keep=True))
    assert np.array_equal(e.h_scale_round(e.to_host(dn), ks, t, ntt=True, plan="two_pass"), rows_engine(e, 0, ks).h_ntt(want()))
    assert np.array_equal(e.to_host(d), a)               # the input is as it was
    return a, want


@pytest.mark.parametrize("lb,nm,ks,t,batch", PLAN_A + PLAN_B + FALLBACK)
def test_every_mode_both_plans_and_the_ntt_form(lb, nm, ks, t, batch, engine_factory):
    e = engine_factory(lb, N, nm)
    a, want = check_shape(e, ks, t, batch)
    # the planted positions reach both sides of both roundings, and the two modes of the first one differ somewhere
    z, Yf = S.stages(a, e.P, ks, t)
    for arr, src in ((z, (0, ks)), (Yf, (ks, nm - ks))):
        _, u, v = B.parts(arr, e.P, src)
        assert set(np.unique((v - u).astype(int)).tolist()) == {0, 1}, src
    assert not np.array_equal(want(), want(floor=True))


def test_u16_words_and_a_misaligned_pointer(engine_factory):
    import torch
    e = engine_factory(16, 4, 2)                       # rows of 8 bytes: the word variant
    check_shape(e, 1, 257, 3, n=4)
    e = engine_factory(64, N, 5)                       # pointers one word past a 16-byte boundary, input and output
    a, want = case(e, 2, 65537, 3)
    buf = torch.zeros(a.size + 1, dtype=torch.int64, device="cuda:0")
    buf[1:].copy_(e.to_device(a).view(-1))
    for keep in (False, True):
        rows = 3 if keep else 2
        out = torch.zeros(3 * rows * N + 2, dtype=torch.int64, device="cuda:0")
        for plan in (None, "two_pass"):
            out.zero_()
            e.scale_round(buf[1:], 2, 65537, keep=keep, out=out[1:-1], plan=plan)
            assert np.array_equal(e.to_host(out[1:-1]).reshape(3, rows, N), want(keep=keep)) and int(out[0]) == 0 and int(out[-1]) == 0


def test_grid_stride_wraps_once(engine_factory):
    """u64/64/5, ks = 2: 32 groups per polynomial, 1024 workgroups of 256 threads -- 8200 polynomials wrap the loop once.  The same
    entry on the batch split in two, and sampled polynomials on both sides of the wrap, the last one included, against the
    restatement."""
    import torch
    e = engine_factory(64, N, 5)
    batch, t = 8200, 65537
    assert batch * N // 2 > 1024 * 256
    d = e.fill_uniform(e.empty(batch), 3, 0)
    got = e.scale_round(d, 2, t)
    half = batch // 2
    assert torch.equal(got[:half], e.scale_round(d[:half].contiguous(), 2, t)) and torch.equal(got[half:], e.scale_round(d[half:].contiguous(), 2, t))
    pick = [0, 1, 8191, 8192, 8193, batch - 1]
    assert np.array_equal(e.to_host(got[pick]), S.scale_round_rns(e.to_host(d[pick]), e.P, 2, t))


def test_graph_capture_replays_identically(engine_factory):
    """one stream, no parallel branches: warm-up calls (they upload the tables and allocate the scratch), then the coefficient form
    and the NTT form captured, both plans"""
    import torch
    e = engine_factory(64, N, 5)
    a, want = case(e, 2, 65537, 3)
    d = e.to_device(a)
    dn = e.ntt_(d.clone())
    fwd = rows_engine(e, 0, 2).h_ntt(want())
    outs = [torch.zeros((3, 2, N), dtype=torch.int64, device="cuda:0") for _ in range(4)]
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()

    def calls():
        e.scale_round(d, 2, 65537, out=outs[0])
        e.scale_round(d, 2, 65537, out=outs[1], plan="two_pass")
        e.scale_round(dn, 2, 65537, ntt=True, out=outs[2])
        e.scale_round(dn, 2, 65537, ntt=True, out=outs[3], plan="two_pass")
    with torch.cuda.stream(st):
        calls()                                           # the warm-up
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            calls()
    for _ in range(3):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(outs[0]), want()) and np.array_equal(e.to_host(outs[1]), want())
        assert np.array_equal(e.to_host(outs[2]), fwd) and np.array_equal(e.to_host(outs[3]), fwd)


def test_the_first_call_while_capturing_is_refused(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e = Engine(64, N, 5, device=0)                        # a context of its own: nothing is warm
    try:
        a, want = case(e, 2, 65537, 3)
        d = e.to_device(a)
        x, z = torch.zeros((3, 2, N), dtype=torch.int64, device="cuda:0"), torch.zeros(4, device="cuda:0")
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        sr, srn = _lib.lib.nflhip_scale_round_dev, _lib.lib.nflhip_scale_round_ntt_dev
        torch.cuda.synchronize()
        # no tables yet; then the tables are there but the two-pass scratch is not; then the NTT form's scratch and child are not
        for fn, flags, warm in ((sr, 0, None), (sr, _lib.SCALE_ROUND_TWO_PASS, 0), (srn, 0, _lib.SCALE_ROUND_TWO_PASS)):
            if warm is not None:
                assert sr(e.ctx, x.data_ptr(), d.data_ptr(), 3, 2, 65537, warm, sp) == 0
                st.synchronize()
                x.zero_()
                torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            rcs = []
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rcs.append(fn(e.ctx, x.data_ptr(), d.data_ptr(), 3, 2, 65537, flags, sp))
            torch.cuda.synchronize()
            assert rcs == [_lib.ERR_UNSUPPORTED], rcs
            assert not x.any()                                   # nothing was enqueued
        assert sr(e.ctx, x.data_ptr(), d.data_ptr(), 3, 2, 65537, 0, sp) == 0      # the same stream, after the captures
        st.synchronize()
        assert np.array_equal(e.to_host(x), want())
    finally:
        e.close()


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    L, ERR = _lib.lib, _lib.ERR_INVALID
    e = engine_factory(64, N, 5)
    d = e.fill_uniform(e.empty(4), 1, 0)
    o = torch.zeros((4, 4, N), dtype=torch.int64, device="cuda:0")
    p, q, row, t = d.data_ptr(), o.data_ptr(), N * 8, 65537
    for fn in (L.nflhip_scale_round_dev, L.nflhip_scale_round_ntt_dev):
        assert fn(None, q, p, 4, 2, t, 0, None) == ERR                            # NULL context
        assert fn(e.ctx, None, p, 4, 2, t, 0, None) == ERR and fn(e.ctx, q, None, 4, 2, t, 0, None) == ERR
        for ks in (0, 5, 6, 2**64 - 1):
            assert fn(e.ctx, q, p, 4, ks, t, 0, None) == ERR, ks                  # ks = 0, ks = nm and beyond
        for bad in (0, 2**61, 2**61 + 1, 2**64 - 1):
            assert fn(e.ctx, q, p, 4, 2, bad, 0, None) == ERR, bad                # t = 0, t >= 2^(limb_bits - 3)
        assert fn(e.ctx, q, p, 4, 2, 2**61 - 1, 0, None) == 0                     # the largest t is served
        for flags in (1, 2, 0x80, 0x800, 0x101, -1):
            assert fn(e.ctx, q, p, 4, 2, t, flags, None) == ERR, flags            # unknown flag bits
        assert fn(e.ctx, p, p, 4, 2, t, 0, None) == ERR                           # in place
        assert fn(e.ctx, p + row, p, 4, 2, t, 0, None) == ERR                     # the output inside the input
        assert fn(e.ctx, p - 8 * row + 8, p, 4, 2, t, 0, None) == ERR             # the output's last word on the input's first
        assert fn(e.ctx, p - 12 * row + 8, p, 4, 2, t, _lib.SCALE_ROUND_KEEP, None) == ERR
        assert fn(e.ctx, q, p, 2**61, 2, t, 0, None) == ERR                       # the size overflows
        assert fn(e.ctx, None, None, 0, 2, t, 0, None) == 0                       # an empty batch is fine ...
        assert fn(e.ctx, None, None, 0, 2, 999983, 0, None) == 0                  # ... and touches nothing: no tables for this t
    e32 = engine_factory(32, N, 5)
    x32 = e32.fill_uniform(e32.empty(1), 1, 0)
    o32 = torch.zeros((1, 2, N), dtype=torch.int32, device="cuda:0")
    assert L.nflhip_scale_round_dev(e32.ctx, o32.data_ptr(), x32.data_ptr(), 1, 2, 2**29, 0, None) == ERR
    assert L.nflhip_scale_round_dev(e32.ctx, o32.data_ptr(), x32.data_ptr(), 1, 2, 2**29 - 1, 0, None) == 0
    h = e.to_host(d)
    ho = np.zeros((4, 2, N), dtype=np.uint64)
    hp = h.ctypes.data
    assert L.nflhip_scale_round(e.ctx, ho.ctypes.data, hp, 4, 5, t, 0) == ERR     # host: ks
    assert L.nflhip_scale_round(e.ctx, None, hp, 4, 2, t, 0) == ERR               # host: NULL
    assert L.nflhip_scale_round(e.ctx, hp + row, hp, 4, 2, t, 0) == ERR           # host: overlap
    assert L.nflhip_scale_round_ntt(e.ctx, ho.ctypes.data, hp, 4, 2, 0, 0) == ERR # host: t
    # a repeated modulus is refused by the table builder, on the host: contexts over moduli 0, 1, 0 (inside S; across S and D)
    from nfllib_amd.params import params
    pr = params(64)
    tabs = [np.ascontiguousarray(x[[0, 1, 0]]) for x in (pr.P, pr.primitive_roots, pr.invkmax)]
    ctx = C.c_void_p()
    assert L.nflhip_ctx_create(C.byref(ctx), 0, 64, N, 3, *[x.ctypes.data_as(C.c_void_p) for x in tabs], pr.kmax_log2) == 0
    try:
        assert L.nflhip_scale_round_dev(ctx, q, p, 1, 1, t, 0, None) == ERR and b"repeats" in L.nflhip_last_error(ctx)
        assert L.nflhip_scale_round_dev(ctx, q, p, 1, 2, t, 0, None) == ERR and b"repeats" in L.nflhip_last_error(ctx)
    finally:
        L.nflhip_ctx_destroy(ctx)
    # nothing refused above wrote anything outside its output, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(d), h)
    o.zero_()
    assert L.nflhip_scale_round_dev(e.ctx, q, p, 4, 2, t, 0, None) == 0
    got = e.to_host(o).reshape(-1)
    assert np.array_equal(got[:4 * 2 * N].reshape(4, 2, N), S.scale_round_rns(h, e.P, 2, t)) and not got[4 * 2 * N:].any()
