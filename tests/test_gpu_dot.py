"""GPU: sums of products across polynomials (nflhip_dot_dev, nflhip_dot_ptrs_dev, nflhip_dot), bit for bit against the Python-
integer restatement of tests/dot_util.py: the lazy accumulator's edges, every limb width, every stride pattern, both plans for a
shared operand, the word path, the pointer form, the host variant, argument checks, graph capture and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dot_util import dot_ref, edge_polys, full_polys, random_polys

pytestmark = pytest.mark.gpu

# the kernel reduces once per 16 terms for every limb width (kernels_dot.hip kDotChunk): a power of two, its neighbours are listed
EDGE_TERMS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65]


def _dev(e, arr):
    return e.to_device(np.ascontiguousarray(arr))


@pytest.mark.parametrize("lb", [64, 32, 16])
def test_lazy_reduction_edge_every_word_p_minus_one(lb, engine_factory):
    n, nm = 64, 2
    e = engine_factory(lb, n, nm)
    full = full_polys(e.P, n, max(EDGE_TERMS), e.np_dtype)
    a, b, add = _dev(e, full), _dev(e, full), _dev(e, full[:1])
    for terms in EDGE_TERMS:
        h = full[:terms][None]
        for addend, hadd in ((None, None), (add, full[:1])):
            got = e.to_host(e.dot(a[:terms], b[:terms], terms, addend=addend))
            assert np.array_equal(got, dot_ref(h, h, e.P, hadd)), (terms, addend is not None)


def test_lazy_reduction_edge_past_the_92nd_modulus(engine_factory):
    lb, n, nm = 64, 1024, 94
    e = engine_factory(lb, n, nm)
    full = full_polys(e.P, n, 17, e.np_dtype)
    a, add = _dev(e, full), _dev(e, full[:1])
    pos = np.unique(np.concatenate([[0, n - 1], np.random.RandomState(2).randint(0, n, 64)]))
    for terms in (8, 9, 17):
        h = full[:terms][None]
        for addend, hadd in ((None, None), (add, full[:1])):
            got = e.to_host(e.dot(a[:terms], a[:terms], terms, addend=addend))
            assert np.array_equal(got[:, 92:], dot_ref(h, h, e.P, hadd, rows=[92, 93])), terms      # delta >= 2^32: whole rows
            assert np.array_equal(got[:, :, pos], dot_ref(h, h, e.P, hadd, positions=pos)), terms


SHAPES = [(64, n, nm) for n in (4, 1024, 4096) for nm in (1, 2, 4)] + [(32, 4096, 3), (32, 4, 2), (16, 128, 2), (16, 4, 1)]


@pytest.mark.parametrize("lb,n,nm", SHAPES)
def test_shapes_groups_and_terms(lb, n, nm, engine_factory):
    """random plus edge inputs, groups in {1, 3, 5} (5 = one full tile of the shared-operand plan and a remainder of 1) x terms
    in {1, 5, 9}: dense, and with the second operand shared.  The products are formed once per shape."""
    e = engine_factory(lb, n, nm)
    ha = edge_polys(e.P, n, 45, e.np_dtype, 11)
    hb = random_polys(e.P, n, 45, e.np_dtype, 12)
    hb[3], hb[4] = full_polys(e.P, n, 1, e.np_dtype)[0], 0
    hadd = edge_polys(e.P, n, 5, e.np_dtype, 13)[::-1].copy()
    prod = ha.astype(object) * hb.astype(object)                    # a[k] * b[k]
    mod = np.array([int(p) for p in e.P], dtype=object)[None, :, None]
    a, b, add = _dev(e, ha), _dev(e, hb), _dev(e, hadd)
    for groups in (1, 3, 5):
        for terms in (1, 5, 9):
            k = groups * terms
            s = prod[:k].reshape(groups, terms, nm, n).sum(axis=1)
            got = e.to_host(e.dot(a[:k], b[:k], terms))
            assert np.array_equal(got, (s % mod).astype(e.np_dtype)), (groups, terms)
            got = e.to_host(e.dot(a[:k], b[:k], terms, addend=add[:groups]))
            assert np.array_equal(got, ((s + hadd[:groups].astype(object)) % mod).astype(e.np_dtype)), (groups, terms, "addend")
            want = dot_ref(ha[:k].reshape(groups, terms, nm, n), hb[:terms], e.P)
            assert np.array_equal(e.to_host(e.matvec(a[:k], b[:terms])), want), (groups, terms, "shared")
            assert np.array_equal(e.to_host(e.matvec(a[:k], b[:terms], untiled=True)), want), (groups, terms, "shared, untiled")


@pytest.mark.parametrize("lb,n,nm", [(64, 1024, 2), (32, 4096, 3), (16, 128, 2)])
def test_strides(lb, n, nm, engine_factory):
    import torch
    e = engine_factory(lb, n, nm)
    groups, terms = 5, 5
    ha = edge_polys(e.P, n, groups * (terms + 2), e.np_dtype, 21)
    hk = random_polys(e.P, n, 2 * terms, e.np_dtype, 22)                       # a key laid out [term][component]
    a, k = _dev(e, ha), _dev(e, hk)
    A = ha[:groups * terms].reshape(groups, terms, nm, n)
    # dense against dense
    hb = random_polys(e.P, n, groups * terms, e.np_dtype, 23)
    assert np.array_equal(e.to_host(e.dot(a[:groups * terms], _dev(e, hb), terms)), dot_ref(A, hb.reshape(groups, terms, nm, n), e.P))
    # b shared: the tiled plan against one group per pass
    tiled = e.matvec(a[:groups * terms], k[:terms])
    untiled = e.matvec(a[:groups * terms], k[:terms], untiled=True)
    assert torch.equal(tiled, untiled)
    assert np.array_equal(e.to_host(tiled), dot_ref(A, hk[:terms], e.P))
    # b = {K + c, 0, 2}
    for c in (0, 1):
        got = e.dot_strided(a, (terms, 1), k[c:], (0, 2), groups, terms)
        assert np.array_equal(e.to_host(got), dot_ref(A, hk[c::2], e.P)), c
        assert torch.equal(got, e.dot_strided(a, (terms, 1), k[c:], (0, 2), groups, terms, untiled=True)), c
    # one shared polynomial: both strides 0
    got = e.dot_strided(a, (terms, 1), k[3:], (0, 0), groups, terms)
    assert np.array_equal(e.to_host(got), dot_ref(A, np.repeat(hk[3:4], terms, axis=0), e.P))
    # a padded matrix: group_stride larger than terms
    got = e.dot_strided(a, (terms + 2, 1), k, (0, 1), groups, terms)
    Ap = ha.reshape(groups, terms + 2, nm, n)[:, :terms]
    assert np.array_equal(e.to_host(got), dot_ref(Ap, hk[:terms], e.P))
    assert torch.equal(got, e.dot_strided(a, (terms + 2, 1), k, (0, 1), groups, terms, untiled=True))
    # the FIRST operand shared: the same sums (the product commutes)
    got = e.dot_strided(k, (0, 1), a, (terms + 2, 1), groups, terms)
    assert np.array_equal(e.to_host(got), dot_ref(Ap, hk[:terms], e.P))


@pytest.mark.parametrize("lb,n,nm", [(64, 1024, 2), (16, 128, 2)])
def test_addend_in_place_and_apart(lb, n, nm, engine_factory):
    e = engine_factory(lb, n, nm)
    groups, terms = 5, 9
    ha, hb = edge_polys(e.P, n, groups * terms, e.np_dtype, 31), random_polys(e.P, n, groups * terms, e.np_dtype, 32)
    hadd = random_polys(e.P, n, groups, e.np_dtype, 33)
    a, b = _dev(e, ha), _dev(e, hb)
    want = dot_ref(ha.reshape(groups, terms, nm, n), hb.reshape(groups, terms, nm, n), e.P, hadd)
    add = _dev(e, hadd)
    assert np.array_equal(e.to_host(e.dot(a, b, terms, addend=add)), want)
    assert np.array_equal(e.to_host(add), hadd)                                # a separate addend is only read
    out = _dev(e, hadd)
    e.dot(a, b, terms, addend=out, out=out)                                    # out += sum
    assert np.array_equal(e.to_host(out), want)
    want_m = dot_ref(ha.reshape(groups, terms, nm, n), hb[:terms], e.P, hadd)
    for untiled in (False, True):
        out = _dev(e, hadd)
        e.matvec(a, b[:terms], addend=out, out=out, untiled=untiled)
        assert np.array_equal(e.to_host(out), want_m), untiled


@pytest.mark.parametrize("lb,n,nm", [(64, 1024, 2), (32, 4096, 3), (16, 128, 2)])
def test_misaligned_operands_take_the_word_path(lb, n, nm, engine_factory):
    """pointers that are not 16-byte aligned (an offset view of a larger buffer) are served word by word, same words"""
    import torch
    e = engine_factory(lb, n, nm)
    groups, terms, w = 3, 5, n * nm
    ha, hb = edge_polys(e.P, n, groups * terms, e.np_dtype, 41), random_polys(e.P, n, terms, e.np_dtype, 42)
    a, b = _dev(e, ha), _dev(e, hb)
    aligned = e.matvec(a, b)
    assert np.array_equal(e.to_host(aligned), dot_ref(ha.reshape(groups, terms, nm, n), hb, e.P))

    def shifted(t):   # the same words, one word further into a larger buffer
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
        buf[1:1 + t.numel()] = t.reshape(-1)
        return buf, buf[1:1 + t.numel()]
    bufa, va = shifted(a)
    bufb, vb = shifted(b)
    bufo = torch.zeros(groups * w + 8, dtype=a.dtype, device=a.device)
    assert va.data_ptr() % 16 != 0
    for untiled in (False, True):
        got = e.dot_strided(va, (terms, 1), b, (0, 1), groups, terms, untiled=untiled)            # one misaligned operand
        assert torch.equal(got, aligned), untiled
        got = e.dot_strided(a, (terms, 1), vb, (0, 1), groups, terms, untiled=untiled)
        assert torch.equal(got, aligned), untiled
        bufo.zero_()
        vo = bufo[1:1 + groups * w]
        e.dot_strided(va, (terms, 1), vb, (0, 1), groups, terms, out=vo, untiled=untiled)         # everything misaligned
        assert torch.equal(vo.reshape(groups, nm, n), aligned), untiled
        assert int(bufo[0]) == 0 and not bufo[1 + groups * w:].any()                               # nothing outside the view


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (32, 1024, 2), (16, 128, 2)])
def test_pointer_form_equals_the_strided_form(lb, n, nm, engine_factory):
    import torch
    e = engine_factory(lb, n, nm)
    ha, hb = edge_polys(e.P, n, 40, e.np_dtype, 51), random_polys(e.P, n, 40, e.np_dtype, 52)
    hadd = random_polys(e.P, n, 1, e.np_dtype, 53)
    # the terms live in separate allocations, in another order than the gathered copy's
    parts_a = [_dev(e, ha[j:j + 1]) for j in range(40)]
    parts_b = [_dev(e, hb[j:j + 1]) for j in reversed(range(40))][::-1]
    a, b, add = _dev(e, ha), _dev(e, hb), _dev(e, hadd)
    for terms in (1, 2, 16, 40):
        want = e.dot(a[:terms], b[:terms], terms)
        assert torch.equal(e.dot_list(parts_a[:terms], parts_b[:terms]), want), terms
        want = e.dot(a[:terms], b[:terms], terms, addend=add)
        assert torch.equal(e.dot_list(parts_a[:terms], parts_b[:terms], addend=add), want), (terms, "addend")
    assert np.array_equal(e.to_host(want), dot_ref(ha[None], hb[None], e.P, hadd))
    out = add.clone()
    e.dot_list(parts_a, parts_b, addend=out, out=out)                          # in place through three chained launches
    assert torch.equal(out, want)


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (32, 1024, 2), (16, 128, 2)])
def test_host_variant_equals_device_variant(lb, n, nm, engine_factory):
    e = engine_factory(lb, n, nm)
    groups, terms = 3, 5
    ha, hb = edge_polys(e.P, n, groups * terms, e.np_dtype, 61), random_polys(e.P, n, groups * terms, e.np_dtype, 62)
    a, b = _dev(e, ha), _dev(e, hb)
    assert np.array_equal(e.h_dot(ha, hb, terms), e.to_host(e.dot(a, b, terms)))
    assert np.array_equal(e.h_dot(ha, hb[:terms], terms, b_shared=True), e.to_host(e.matvec(a, b[:terms])))


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (32, 1024, 2), (16, 128, 2)])
def test_compiled_variant_equals_default(lb, n, nm, engine_factory, compiled_engine_factory):
    import torch
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    groups, terms = 5, 17
    a, b = e.fill_uniform(e.empty(groups * terms), 71, 0), e.fill_uniform(e.empty(groups * terms), 72, 1)
    assert torch.equal(c.dot(a, b, terms), e.dot(a, b, terms))
    assert torch.equal(c.matvec(a, b[:terms]), e.matvec(a, b[:terms]))
    assert torch.equal(c.dot_list(list(a[:16].split(1)), list(b[:16].split(1))), e.dot(a[:16], b[:16], 16))


def test_larger_run_u64_4096_4(engine_factory):
    """groups 256 x terms 16: six sampled groups against the restatement (64 sampled positions of every row, the first and the
    last row whole), every group against the same call on slices of 16 groups, compared on the device"""
    import torch
    lb, n, nm, groups, terms = 64, 4096, 4, 256, 16
    e = engine_factory(lb, n, nm)
    a = e.fill_uniform(e.empty(groups * terms), 81, 0)
    b = e.fill_uniform(e.empty(groups * terms), 82, 1)
    out = e.dot(a, b, terms)
    mv, mvu = e.matvec(a, b[:terms]), e.matvec(a, b[:terms], untiled=True)
    assert torch.equal(mv, mvu)
    for g0 in range(0, groups, 16):
        s = slice(g0 * terms, (g0 + 16) * terms)
        assert torch.equal(e.dot(a[s], b[s], terms), out[g0:g0 + 16]), g0
        assert torch.equal(e.matvec(a[s], b[:terms]), mv[g0:g0 + 16]), g0
    pos = np.unique(np.concatenate([[0, n - 1], np.random.RandomState(3).randint(0, n, 64)]))
    hv = e.to_host(b[:terms])
    for g in (0, 1, 77, 128, 254, 255):
        s = slice(g * terms, (g + 1) * terms)
        ha, hb, got, gotm = e.to_host(a[s])[None], e.to_host(b[s])[None], e.to_host(out[g:g + 1]), e.to_host(mv[g:g + 1])
        assert np.array_equal(got[:, :, pos], dot_ref(ha, hb, e.P, positions=pos)), g
        assert np.array_equal(got[:, [0, nm - 1]], dot_ref(ha, hb, e.P, rows=[0, nm - 1])), g
        assert np.array_equal(gotm[:, :, pos], dot_ref(ha, hv, e.P, positions=pos)), g


def test_invalid_arguments(engine_factory):
    """every refusal of include/nflhip.h "sums of products" (a cyclic row context cannot be reached through the public entries),
    the boundaries of the overlap rule from both sides, and that nothing was written"""
    import torch
    from nfllib_amd import _lib
    L, ERR, Op = _lib.lib, _lib.ERR_INVALID, _lib.DotOperand
    e = engine_factory(64, 1024, 2)
    groups, terms = 2, 3
    buf = e.fill_uniform(e.empty(18), 1, 0)       # polynomials: a = [0, 6), b = [6, 12), out = [12, 14), spare = [14, 18)
    h = e.to_host(buf).copy()
    pb = 2 * 1024 * 8                             # bytes per polynomial
    pa = buf.data_ptr()
    pbb, po = pa + 6 * pb, pa + 12 * pb
    A, B = Op(pa, terms, 1), Op(pbb, terms, 1)

    def call(out, a, b, add=None, g=groups, t=terms, flags=0, ctx=e.ctx):
        return L.nflhip_dot_dev(ctx, out, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, add, g, t, flags, None)
    assert call(po, A, B, ctx=None) == ERR                                   # NULL context
    assert call(None, A, B) == ERR                                           # NULL output
    assert call(po, None, B) == ERR and call(po, A, None) == ERR             # NULL operand record
    assert call(po, Op(None, terms, 1), B) == ERR and call(po, A, Op(None, terms, 1)) == ERR   # NULL operand pointer
    assert call(po, A, B, t=0) == ERR                                        # no terms
    for t in (2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1):               # past the kernel's 32-bit term counter: with both
        assert call(po, Op(pa, 0, 0), Op(pbb, 0, 0), t=t) == ERR             # strides 0 such a call would need no memory
    for flags in (1, 0x200, 0x101, -1):
        assert call(po, A, B, flags=flags) == ERR                            # unknown flag bits
    assert call(pa, A, B) == ERR and call(pbb, A, B) == ERR                  # in place
    assert call(pa + pb, A, B) == ERR                                        # the output inside a
    assert call(pa - groups * pb + 8, A, B) == ERR                           # the output's last word on a's first
    assert call(po, Op(po + 8 - 6 * pb, terms, 1), B) == ERR                 # a's last word on the output's first
    assert call(po, A, Op(po + 8 - 6 * pb, terms, 1)) == ERR                 # b's last word on the output's first
    assert call(pbb + terms * pb - 8, A, Op(pbb, 0, 1)) == ERR               # a shared vector ends `terms` polynomials after its pointer
    assert call(po, Op(pa, 10, 1), B) == ERR                                 # a padded matrix reaches (groups - 1) * 10 + terms = 13 polynomials
    assert call(po, A, B, add=po + 8) == ERR and call(po, A, B, add=po - pb) == ERR and call(po, A, B, add=po + groups * pb - 8) == ERR   # an addend that overlaps the output, not exactly
    P1 = (C.c_void_p * 17)(*[pa + (j % 6) * pb for j in range(17)])
    P2 = (C.c_void_p * 17)(*[pbb + (j % 6) * pb for j in range(17)])
    ptr = L.nflhip_dot_ptrs_dev
    assert ptr(None, po, P1, P2, 3, None, None) == ERR
    assert ptr(e.ctx, None, P1, P2, 3, None, None) == ERR and ptr(e.ctx, po, None, P2, 3, None, None) == ERR and ptr(e.ctx, po, P1, None, 3, None, None) == ERR
    assert ptr(e.ctx, po, P1, P2, 0, None, None) == ERR and ptr(e.ctx, po, P1, P2, 17, None, None) == ERR
    assert ptr(e.ctx, pa + 2 * pb, P1, P2, 3, None, None) == ERR             # the output is a term
    assert ptr(e.ctx, pa + 3 * pb - 8, P1, P2, 3, None, None) == ERR         # its first word on a term's last
    assert ptr(e.ctx, pa - pb + 8, P1, P2, 3, None, None) == ERR             # its last word on a term's first
    assert ptr(e.ctx, po, P1, P2, 3, po + 8, None) == ERR                    # an addend that overlaps, not exactly
    Pn = (C.c_void_p * 3)(pa, None, pa + pb)
    assert ptr(e.ctx, po, Pn, P2, 3, None, None) == ERR                      # a NULL term
    hp, ho = h.ctypes.data, np.zeros((groups, 2, 1024), dtype=np.uint64)
    assert L.nflhip_dot(None, ho.ctypes.data, hp, hp, groups, terms, 0) == ERR
    assert L.nflhip_dot(e.ctx, None, hp, hp, groups, terms, 0) == ERR and L.nflhip_dot(e.ctx, ho.ctypes.data, None, hp, groups, terms, 0) == ERR
    assert L.nflhip_dot(e.ctx, ho.ctypes.data, hp, None, groups, terms, 0) == ERR
    assert L.nflhip_dot(e.ctx, ho.ctypes.data, hp, hp, groups, 0, 0) == ERR
    assert L.nflhip_dot(e.ctx, hp + pb, hp, hp + 6 * pb, groups, terms, 0) == ERR          # host: the output overlaps a
    assert call(None, A, B, g=0) == 0 and L.nflhip_dot(e.ctx, None, None, None, 0, terms, 0) == 0   # no groups: fine, nothing touched
    # nothing above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(buf), h) and not ho.any()
    Ah = h[:6].reshape(groups, terms, 2, 1024)
    # valid: the output starts where a shared vector's extent ends (polynomials [9, 11)) ...
    assert call(pbb + terms * pb, A, Op(pbb, 0, 1)) == 0
    torch.cuda.synchronize()
    got = e.to_host(buf).copy()
    assert np.array_equal(got[9:11], dot_ref(Ah, h[6:9], e.P))
    assert np.array_equal(got[:9], h[:9]) and np.array_equal(got[11:], h[11:])
    # ... a padded matrix that reaches exactly the output's first byte, (groups - 1) * 9 + terms = 12 polynomials ...
    assert call(po, Op(pa, 9, 1), B) == 0
    torch.cuda.synchronize()
    got2 = e.to_host(buf).copy()
    Ap = np.stack([got[0:3], got[9:12]])
    assert np.array_equal(got2[12:14], dot_ref(Ap, got[6:12].reshape(groups, terms, 2, 1024), e.P))
    # ... and adjacent buffers: a ends where b starts, b ends where the output starts, the addend follows the output
    assert call(po, A, B, add=po + groups * pb) == 0
    torch.cuda.synchronize()
    got3 = e.to_host(buf)
    assert np.array_equal(got3[12:14], dot_ref(Ah, got[6:12].reshape(groups, terms, 2, 1024), e.P, got[14:16]))
    assert np.array_equal(got3[:12], got[:12]) and np.array_equal(got3[14:], h[14:])


def test_graph_capture_replays_identically(engine_factory):
    """the strided form (both plans) and the pointer form at u64/4096/4: no scratch, no allocation, capturable"""
    import torch
    e = engine_factory(64, 4096, 4)
    groups, terms = 5, 9
    ha, hb = edge_polys(e.P, 4096, groups * terms, e.np_dtype, 91), random_polys(e.P, 4096, groups * terms, e.np_dtype, 92)
    a, b = _dev(e, ha), _dev(e, hb)
    A = ha.reshape(groups, terms, 4, 4096)
    want = dot_ref(A, hb.reshape(groups, terms, 4, 4096), e.P)
    want_m = dot_ref(A, hb[:terms], e.P)
    parts_a, parts_b = list(a[:terms].split(1)), list(b[:terms].split(1))
    x, y, z = e.empty(groups), e.empty(groups), e.empty(1)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()

    def work():
        e.dot(a, b, terms, out=x)
        e.matvec(a, b[:terms], out=y)
        e.dot_list(parts_a, parts_b, out=z)
    with torch.cuda.stream(st):
        work()
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            work()
    for _ in range(3):
        for t in (x, y, z):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(x), want)
        assert np.array_equal(e.to_host(y), want_m)
        assert np.array_equal(e.to_host(z), want[:1])


@pytest.fixture(scope="module")
def cpp_programs(tmp_path_factory):
    from test_dot_cpu import build_cpp
    out = str(tmp_path_factory.mktemp("cpp_dot"))
    return build_cpp(out), build_cpp(out, eager=True)


@pytest.mark.parametrize("mode", ["thread0", "thread1", "eager_runtime", "eager_build"])
def test_cpp_surface_on_the_gpu(mode, cpp_programs):
    """poly, poly_p (deferred operations pending before the call and recorded after it), device_batch::assign_dot and
    assign_matvec -- under both queue executors and with deferred execution off"""
    exe = cpp_programs[1] if mode == "eager_build" else cpp_programs[0]
    env = dict(os.environ)
    env["NFL_HIP_QUEUE_THREAD"] = "0" if mode == "thread0" else "1"
    args = [exe] + (["eager"] if mode == "eager_runtime" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
