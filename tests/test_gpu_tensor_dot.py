"""GPU: the tensor product summed over terms (include/nflhip.h "sums of ciphertext products", nfllib_amd/csrc/kernels_tensor_dot.hip).
Every word against tests/mulrelin_dot_util.tensor_dot_rns (Python integers) and against the same sums composed from
Engine(lb, n, rows).dot_strided -- four sums of products, the cross sum through the addend.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from mulrelin_dot_util import operand, tensor_dot_rns

pytestmark = pytest.mark.gpu


def blocks(e, rows, count, seed, n=None):
    return [B.random_batch(e.P[:rows], e.degree, count, e.np_dtype, seed + t) for t in range(4)]


def composed(er, ops, groups, terms):
    """(D0, D1, D2) through dot_strided on the engine over the first `rows` moduli; ops = four (tensor, strides), b = a for the squares"""
    (a0, s0), (a1, s1), (b0, t0), (b1, t1) = ops
    D0 = er.dot_strided(a0, s0, b0, t0, groups, terms)
    D1 = er.dot_strided(a0, s0, b1, t1, groups, terms)
    er.dot_strided(a1, s1, b0, t0, groups, terms, addend=D1, out=D1)
    D2 = er.dot_strided(a1, s1, b1, t1, groups, terms)
    return D0, D1, D2


def check(e, er, rows, groups, terms, square, shared, seed=5, host=True):
    import torch
    n = e.degree
    h = blocks(e, rows, groups * terms, seed)
    if shared:
        h[2], h[3] = h[2][:terms].copy(), h[3][:terms].copy()
    d = [e.to_device(x) for x in h]
    hb = (None, None) if square else (operand(h[2], groups, terms, shared), operand(h[3], groups, terms, shared))
    want = tensor_dot_rns(operand(h[0], groups, terms), operand(h[1], groups, terms), hb[0], hb[1], e.P)
    got = e.tensor_dot_ntt(d[0], d[1], None if square else d[2], None if square else d[3], terms=terms, rows=rows, b_shared=shared)
    sa, sb = (terms, 1), (0 if shared else terms, 1)
    ops = [(d[0], sa), (d[1], sa)] + ([(d[0], sa), (d[1], sa)] if square else [(d[2], sb), (d[3], sb)])
    comp = composed(er, ops, groups, terms)
    for g, c, w in zip(got, comp, want):
        assert g.shape == (groups, rows, n)
        assert np.array_equal(e.to_host(g), w), (rows, groups, terms, square, shared)
        assert torch.equal(g.reshape(-1), c.reshape(-1))
    if host:
        hv = e.h_tensor_dot_ntt(h[0], h[1], None if square else h[2], None if square else h[3], terms=terms, rows=rows, b_shared=shared)
        for g, w in zip(hv, want):
            assert np.array_equal(g, w)
    for x, y in zip(d, h):
        assert np.array_equal(e.to_host(x), y)                                   # the operands are only read


@pytest.mark.parametrize("lb,n,nm,rows", [(64, 64, 4, 4), (64, 64, 4, 3), (32, 128, 3, 3), (32, 128, 3, 2), (16, 4, 2, 2), (16, 4, 2, 1)])
def test_against_the_integers_and_the_dot_composition(lb, n, nm, rows, engine_factory):
    """rows = nm and rows < nm; general and square; dense and shared b; 3 groups of 5 terms (an odd count: the prefetched term is
    the last one in an odd and an even position) and 1 group of 2; rows of 8 bytes (u16/4: the word variant)"""
    e, er = engine_factory(lb, n, nm), engine_factory(lb, n, rows)
    for groups, terms in ((3, 5), (1, 2)):
        for square in (False, True):
            for shared in ((False,) if square else (False, True)):
                check(e, er, rows, groups, terms, square, shared)


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 4), (32, 128, 3), (16, 4, 2)])
def test_a_key_like_layout_with_term_stride_two(lb, n, nm, engine_factory):
    """b0 and b1 interleaved as a key's two columns are: [terms][2][rows][n], shared by every group, term stride 2"""
    e = engine_factory(lb, n, nm)
    groups, terms = 3, 4
    h = blocks(e, nm, groups * terms, 21)
    key = B.random_batch(e.P, n, 2 * terms, e.np_dtype, 29).reshape(terms, 2, nm, n)
    d, dk = [e.to_device(x) for x in h[:2]], e.to_device(key)
    poly = nm * n * e.np_dtype.itemsize
    got = e.tensor_dot_strided((d[0], (terms, 1)), (d[1], (terms, 1)), (dk.data_ptr(), (0, 2)), (dk.data_ptr() + poly, (0, 2)), groups, terms)
    want = tensor_dot_rns(operand(h[0], groups, terms), operand(h[1], groups, terms), operand(key[:, 0], groups, terms, True),
                          operand(key[:, 1], groups, terms, True), e.P)
    comp = composed(e, [(d[0], (terms, 1)), (d[1], (terms, 1)), (dk.data_ptr(), (0, 2)), (dk.data_ptr() + poly, (0, 2))], groups, terms)
    for g, c, w in zip(got, comp, want):
        assert np.array_equal(e.to_host(g), w) and np.array_equal(e.to_host(c), w)


def test_the_moduli_at_which_a_late_reduction_wraps():
    """on the moduli table: for the first 64- and 32-bit moduli nine terms of two products, and seventeen single products, of (p - 1)^2
    already exceed 2^(2W) -- a sum reduced one term late wraps there.  The two 14-bit moduli wrap only from 19 and 25 products on, so
    at u16 only terms = 33 (33 single products, 66 cross products) bites."""
    from nfllib_amd.params import params
    for lb in (64, 32):
        p = int(params(lb).P[0])
        assert 18 * (p - 1) ** 2 >= 2 ** (2 * lb) and 17 * (p - 1) ** 2 >= 2 ** (2 * lb)
        assert 16 * (p - 1) ** 2 + p - 1 < 2 ** (2 * lb)
    first = [-(-2 ** 32 // (int(p) - 1) ** 2) for p in params(16).P[:2]]
    assert sorted(first) == [19, 25], first


@pytest.mark.parametrize("terms", [7, 8, 9, 16, 17, 33])
@pytest.mark.parametrize("lb,n,nm", [(64, 64, 4), (32, 128, 3), (16, 4, 2)])
def test_accumulator_edges(lb, n, nm, terms, engine_factory):
    """every operand word p_m - 1: the largest sums the accumulators see, at the term counts around the two reduction cadences (D1
    every 8 terms, D0 and D2 every 16).  General and square, vector and word variant (one operand a word off 16 bytes)."""
    import torch
    e = engine_factory(lb, n, nm)
    groups = 2
    top = np.empty((groups * terms, nm, n), dtype=e.np_dtype)
    for m, p in enumerate(e.P):
        top[:, m] = p - 1
    x = operand(top, groups, terms)
    d = e.to_device(top)
    off = torch.zeros(top.size + 1, dtype=e.torch_dtype, device="cuda:0")
    off[1:].copy_(d.view(-1))
    for square in (False, True):
        want = tensor_dot_rns(x, x, None if square else x, None if square else x, e.P)
        for m, p in enumerate(e.P):                                              # ((p - 1)^2 = 1: the sums are the counts)
            assert int(want[0][0, m, 0]) == terms % p and int(want[1][0, m, 0]) == 2 * terms % p
        b = (None, None) if square else (d, d)
        for a0 in (d, off[1:]):
            got = e.tensor_dot_ntt(a0, d, b[0], b[1], terms=terms)
            for g, w in zip(got, want):
                assert np.array_equal(e.to_host(g), w), (terms, square, a0 is d)


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 4), (32, 128, 3)])
def test_one_pointer_a_word_off_with_guard_words_around_the_outputs(lb, n, nm, engine_factory):
    import torch
    e = engine_factory(lb, n, nm)
    groups, terms, V = 2, 3, 16 // e.np_dtype.itemsize
    h = blocks(e, nm, groups * terms, 33)
    want = tensor_dot_rns(*[operand(x, groups, terms) for x in h], e.P)
    d = [e.to_device(x) for x in h]
    buf = torch.zeros(h[1].size + 2, dtype=e.torch_dtype, device="cuda:0")
    buf[1:-1].copy_(d[1].view(-1))                                               # a1 alone is a word off
    size = groups * nm * n
    outs = [torch.full((size + 2 * V,), 7, dtype=e.torch_dtype, device="cuda:0") for _ in range(3)]
    e.tensor_dot_ntt(d[0], buf[1:-1], d[2], d[3], terms=terms, outs=[o[V:-V] for o in outs])
    for o, w in zip(outs, want):
        assert np.array_equal(e.to_host(o[V:-V]).reshape(w.shape), w)
        assert bool((o[:V] == 7).all()) and bool((o[-V:] == 7).all())
    outs = [torch.full((size + 2,), 7, dtype=e.torch_dtype, device="cuda:0") for _ in range(3)]   # and the outputs a word off
    e.tensor_dot_ntt(d[0], d[1], d[2], d[3], terms=terms, outs=[o[1:-1] for o in outs])
    for o, w in zip(outs, want):
        assert np.array_equal(e.to_host(o[1:-1]).reshape(w.shape), w) and int(o[0]) == 7 and int(o[-1]) == 7
    assert int(buf[0]) == 0 and int(buf[-1]) == 0


@pytest.mark.parametrize("lb,n,nm,groups,terms", [(16, 4, 2, 262147, 2), (32, 128, 3, 10923, 1)])
def test_a_count_that_wraps_the_grid_stride_loop(lb, n, nm, groups, terms, engine_factory):
    """the grid is bounded at 4096 workgroups over all rows: u16/4/2 (words) 2048 x 256 threads per row against 4 x 262147 words;
    u32/128/3 (16-byte groups) 1365 x 256 against 32 x 10923 groups.  The reference is exact 64-bit arithmetic: the sums of two or
    four products of these words stay below 2^64."""
    e = engine_factory(lb, n, nm)
    h = [B.random_batch(e.P, n, groups * terms, e.np_dtype, 41 + t) for t in range(4)]
    x0, x1, y0, y1 = (operand(x, groups, terms).astype(np.uint64) for x in h)
    P = np.array(e.P, dtype=np.uint64)[None, :, None]
    want = [((x0 * y0).sum(axis=1) % P), ((x0 * y1 + x1 * y0).sum(axis=1) % P), ((x1 * y1).sum(axis=1) % P)]
    got = e.tensor_dot_ntt(*[e.to_device(x) for x in h], terms=terms)
    for g, w in zip(got, want):
        assert np.array_equal(e.to_host(g).astype(np.uint64), w)


def test_one_group_is_group_zero_of_three_and_no_group_is_nothing(engine_factory):
    import torch
    from nfllib_amd import _lib
    e = engine_factory(64, 64, 4)
    terms = 3
    h = blocks(e, 4, 3 * terms, 51)
    d = [e.to_device(x) for x in h]
    three = e.tensor_dot_ntt(*d, terms=terms)
    one = e.tensor_dot_ntt(*[x[:terms].contiguous() for x in d], terms=terms)
    for a, b in zip(one, three):
        assert a.shape[0] == 1 and torch.equal(a[0], b[0])
    ops = [_lib.DotOperand(x.data_ptr(), terms, 1) for x in d]
    r = [C.byref(o) for o in ops]
    assert _lib.lib.nflhip_tensor_dot_ntt_dev(e.ctx, None, None, None, r[0], r[1], r[2], r[3], 0, terms, 4, 0, None) == 0
    assert _lib.lib.nflhip_tensor_dot_ntt(e.ctx, None, None, None, None, None, None, None, 0, terms, 0, 4, 0) == 0


def test_every_refusal_comes_before_the_device_is_touched(engine_factory):
    import torch
    from nfllib_amd import _lib
    e = engine_factory(64, 64, 4)
    groups, terms, rows = 2, 3, 4
    pb = rows * 64 * 8
    big = torch.full((16 * groups * terms * rows * 64,), 9, dtype=torch.int64, device="cuda:0")
    blk = groups * terms * pb
    p = [big.data_ptr() + k * blk for k in range(8)]
    T, ERR = _lib.lib.nflhip_tensor_dot_ntt_dev, _lib.ERR_INVALID

    def op(ptr, gs=terms, ts=1):
        return _lib.DotOperand(ptr, gs, ts)

    def call(outs, ops, groups=groups, terms=terms, rows=rows, flags=0, ctx=e.ctx):
        refs = [None if o is None else C.byref(o) for o in ops]
        return T(ctx, outs[0], outs[1], outs[2], refs[0], refs[1], refs[2], refs[3], groups, terms, rows, flags, None)

    good_o, good = (p[0], p[1], p[2]), [op(p[3]), op(p[4]), op(p[5]), op(p[6])]
    assert call(good_o, good) == 0
    torch.cuda.synchronize()
    big.fill_(9)
    ob = groups * pb
    for outs in ((None, p[1], p[2]), (p[0], None, p[2]), (p[0], p[1], None),                       # a NULL output
                 (p[0], p[0], p[2]), (p[0], p[1], p[1] + ob - 8),                                   # two outputs overlap
                 (p[3] + blk - 8, p[1], p[2]), (p[0], p[1], p[6]), (p[0], p[4] + 8, p[2])):          # an output on an operand's bytes
        assert call(outs, good) == ERR, outs
    for ops in ([None, good[1], good[2], good[3]], [good[0], None, good[2], good[3]],               # a NULL operand
                [good[0], good[1], None, good[3]], [good[0], good[1], good[2], None],               # exactly one of b0 / b1
                [op(None), good[1], good[2], good[3]], [good[0], good[1], good[2], op(None)],       # a NULL pointer inside
                [op(p[3], 2**62, 1), good[1], good[2], good[3]], [good[0], good[1], op(p[5], 0, 2**63), good[3]],   # an extent that overflows
                [good[0], good[1], good[2], op(p[0] - (terms - 1) * pb, 0, 1)]):                    # the last term of a shared b1 under out0
        assert call(good_o, ops) == ERR
    # the extent rule: a shared b of `terms` polynomials right below out0 is apart from it, one polynomial further on is not
    assert call((p[1], p[2], p[7]), [good[0], good[1], op(p[1] - terms * pb, 0, 1), good[3]]) == 0
    torch.cuda.synchronize()
    big.fill_(9)
    for kw in (dict(terms=0), dict(terms=2**31 + 1), dict(rows=0), dict(rows=5), dict(flags=1), dict(flags=0x100), dict(groups=2**61), dict(ctx=None)):
        assert call(good_o, good, **kw) == ERR, kw
    # (a cyclic row context cannot be reached through the public entries: tests/test_gpu_dot.py)
    torch.cuda.synchronize()
    assert bool((big == 9).all())                                                # nothing refused wrote anything


def test_one_capture_on_one_stream_replays_identically(engine_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e = engine_factory(64, 64, 4)
    groups, terms = 3, 9
    h = blocks(e, 4, groups * terms, 61)
    want = tensor_dot_rns(*[operand(x, groups, terms) for x in h], e.P)
    d = [e.to_device(x) for x in h]
    o = torch.zeros((3, groups, 4, 64), dtype=torch.int64, device="cuda:0")
    outs = (o[0], o[1], o[2])

    def run():
        e.tensor_dot_ntt(*d, terms=terms, outs=outs)

    def ok():
        return all(np.array_equal(e.to_host(g), w) for g, w in zip(outs, want))

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        run()
        st.synchronize()
        assert ok()
        with torch.cuda.graph(g, stream=st):
            run()
    for _ in range(3):
        o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ok()
