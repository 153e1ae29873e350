"""GPU: several outputs against one first operand (nflhip_dot_multi_dev, nfllib_amd/csrc/kernels_dot_multi.hip).  Every case is
checked against the per-output nflhip_dot_dev result AND the Python-integer sum of tests/dot_util.py: the register form's last
size (8 terms), the streaming form's first (9), a crossing of the 16-term chunk (17); 1, 2 and 32 outputs; groups with a tile
remainder; the word variant; misaligned pointers; both layouts of the digits of a hoisted rotation; argument checks; capture."""
import ctypes as C

import numpy as np
import pytest

from dot_util import dot_ref, edge_polys, full_polys, random_polys

pytestmark = pytest.mark.gpu

TERMS = [1, 8, 9, 17]
_CACHE = {}


def _dev(e, arr):
    return e.to_device(np.ascontiguousarray(arr))


def operands(e, n):
    """a = 5 x 17 polynomials with the edge words (0, p - 1, mixes), b = 32 + 16 polynomials, one of them every word p - 1, one 0;
    computed once per shape"""
    key = (e.limb_bits, n, e.nmoduli)
    if key not in _CACHE:
        ha = edge_polys(e.P, n, 5 * 17, e.np_dtype, 41)
        hb = random_polys(e.P, n, 32 + 16, e.np_dtype, 42)
        hb[3], hb[4] = full_polys(e.P, n, 1, e.np_dtype)[0], 0
        _CACHE[key] = (ha, hb)
    return _CACHE[key]


def check(e, n, groups, terms, outputs, untiled=False):
    import torch
    nm = e.nmoduli
    ha, hb = operands(e, n)
    a, b = _dev(e, ha), _dev(e, hb)
    # a = [groups][terms] dense; b_o(j) = hb[o + j]: the second operands overlap each other, which is allowed
    bs = [b[o:] for o in range(outputs)]
    got = e.dot_multi(a, (terms, 1), bs, 1, groups, terms, untiled=untiled)
    A = ha[:groups * terms].reshape(groups, terms, nm, n)
    for o in range(outputs):
        one = e.dot_strided(a, (terms, 1), bs[o], (0, 1), groups, terms)
        assert torch.equal(got[o], one), (groups, terms, outputs, o, untiled)
        assert np.array_equal(e.to_host(got[o]), dot_ref(A, hb[o:o + terms], e.P)), (groups, terms, outputs, o, untiled)


@pytest.mark.parametrize("terms", TERMS)
def test_terms_outputs_and_groups(terms, engine_factory):
    e = engine_factory(64, 64, 3)
    for outputs in (1, 2, 32):
        for groups in (1, 3, 5):
            check(e, 64, groups, terms, outputs)


@pytest.mark.parametrize("lb,n,nm", [(32, 128, 2), (16, 4, 2)])
def test_other_limb_widths_and_the_word_variant(lb, n, nm, engine_factory):
    """u16/4: rows of 8 bytes, below one 16-byte group"""
    e = engine_factory(lb, n, nm)
    for terms in TERMS:
        for outputs, groups in ((1, 1), (2, 3), (32, 5)):
            check(e, n, groups, terms, outputs)


@pytest.mark.parametrize("terms", [8, 9])
def test_untiled_equals_tiled(terms, engine_factory):
    import torch
    e = engine_factory(64, 64, 3)
    ha, hb = operands(e, 64)
    a, b = _dev(e, ha), _dev(e, hb)
    bs = [b[o:] for o in range(4)]
    for groups in (1, 3, 5):
        t, u = e.dot_multi(a, (terms, 1), bs, 1, groups, terms), e.dot_multi(a, (terms, 1), bs, 1, groups, terms, untiled=True)
        for o in range(4):
            assert torch.equal(t[o], u[o]), (groups, o)
        check(e, 64, groups, terms, 4, untiled=True)


@pytest.mark.parametrize("terms", [8, 9])
def test_every_pointer_one_word_off_alignment_with_guard_words(terms, engine_factory):
    import torch
    e = engine_factory(64, 64, 3)
    nm, n, groups, outputs = 3, 64, 3, 3
    ha, hb = operands(e, n)
    na, nb, no = groups * terms * nm * n, (terms + 1) * nm * n, groups * nm * n
    a = torch.zeros(na + 2, dtype=torch.int64, device="cuda:0")
    a[1:-1].copy_(_dev(e, ha[:groups * terms]).view(-1))
    bs = []
    for o in range(outputs):
        t = torch.zeros(nb + 2, dtype=torch.int64, device="cuda:0")
        t[1:-1].copy_(_dev(e, hb[o:o + terms + 1]).view(-1))
        bs.append(t)
    outs = [torch.full((no + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(outputs)]
    e.dot_multi(a[1:-1], (terms, 1), [t[1:-1] for t in bs], 1, groups, terms, outs=[o[1:-1] for o in outs])
    A = ha[:groups * terms].reshape(groups, terms, nm, n)
    for o in range(outputs):
        assert np.array_equal(e.to_host(outs[o][1:-1]).reshape(groups, nm, n), dot_ref(A, hb[o:o + terms], e.P)), o
        assert int(outs[o][0]) == 7 and int(outs[o][-1]) == 7
    assert int(a[0]) == 0 and int(a[-1]) == 0 and all(int(t[0]) == 0 and int(t[-1]) == 0 for t in bs)


def test_strided_a_in_both_layouts_of_the_digits(engine_factory):
    """U = [dnum][batch] read with strides (1, batch), U = [batch][dnum] with (dnum, 1); b = a key [term][component], term stride 2"""
    import torch
    e = engine_factory(64, 64, 3)
    nm, n, batch, dnum = 3, 64, 5, 3
    ha, hb = operands(e, n)
    a, k = _dev(e, ha), _dev(e, hb)
    U = ha[:batch * dnum]
    for strides, A in (((1, batch), U.reshape(dnum, batch, nm, n).transpose(1, 0, 2, 3)), ((dnum, 1), U.reshape(batch, dnum, nm, n))):
        bs = [k[c:] for c in range(4)]                                     # two keys' worth of components
        got = e.dot_multi(a, strides, bs, 2, batch, dnum)
        for c in range(4):
            assert np.array_equal(e.to_host(got[c]), dot_ref(A, hb[c::2][:dnum], e.P)), (strides, c)
            assert torch.equal(got[c], e.dot_strided(a, strides, k[c:], (0, 2), batch, dnum)), (strides, c)


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    Lb, ERR = _lib.lib, _lib.ERR_INVALID
    e = engine_factory(64, 64, 3)
    pb, groups, terms = 3 * 64 * 8, 2, 3
    a = torch.ones((groups * terms, 3, 64), dtype=torch.int64, device="cuda:0")
    b = torch.ones((2 * terms, 3, 64), dtype=torch.int64, device="cuda:0")
    o = torch.full((2, groups, 3, 64), 9, dtype=torch.int64, device="cuda:0")
    f = Lb.nflhip_dot_multi_dev

    def call(ctx, outs, aptr, bs, b_ts=1, outputs=None, g=groups, t=terms, flags=0, a_strides=(terms, 1)):
        po = (C.c_void_p * 33)(*outs) if outs is not None else None
        pbs = (C.c_void_p * 33)(*bs) if bs is not None else None
        op = C.byref(_lib.DotOperand(aptr, *a_strides)) if aptr != "null" else None
        return f(ctx, po, op, pbs, b_ts, len(outs) if outputs is None else outputs, g, t, flags, None)

    pa, pk, p0, p1 = a.data_ptr(), b.data_ptr(), o[0].data_ptr(), o[1].data_ptr()
    ok = ([p0, p1], pa, [pk, pk + terms * pb])
    assert call(None, *ok) == ERR                                                       # NULL context
    assert call(e.ctx, None, pa, ok[2], outputs=2) == ERR and call(e.ctx, ok[0], pa, None, outputs=2) == ERR
    assert call(e.ctx, ok[0], "null", ok[2]) == ERR and call(e.ctx, ok[0], None, ok[2]) == ERR   # no operand; a NULL ptr
    assert call(e.ctx, [p0, None], pa, ok[2]) == ERR and call(e.ctx, ok[0], pa, [pk, None]) == ERR
    assert call(e.ctx, ok[0], pa, ok[2], outputs=0) == ERR
    assert call(e.ctx, [p0] * 33, pa, [pk] * 33, outputs=33) == ERR                    # more than 32 outputs
    assert call(e.ctx, *ok, t=0) == ERR and call(e.ctx, *ok, t=2**31 + 1) == ERR
    for flags in (1, 0x200, -1):
        assert call(e.ctx, *ok, flags=flags) == ERR, flags
    assert call(e.ctx, *ok, g=2**61) == ERR and call(e.ctx, *ok, b_ts=2**62) == ERR and call(e.ctx, *ok, a_strides=(2**62, 1)) == ERR   # overflow
    obytes = groups * pb
    assert call(e.ctx, [p0, p0], pa, ok[2]) == ERR and call(e.ctx, [p0, p0 + obytes - 8], pa, ok[2]) == ERR   # two outputs overlap
    assert call(e.ctx, [p0, pa + (groups * terms - 1) * pb], pa, ok[2]) == ERR           # an output on a's last polynomial
    assert call(e.ctx, [pk + (2 * terms - 1) * pb - obytes + 8, p1], pa, ok[2]) == ERR   # output 0 on the last word of b_1's extent
    assert call(e.ctx, [p0, pk - obytes + 8], pa, ok[2]) == ERR                          # output 1 on the first word of b_0
    assert call(e.ctx, [p0, p1], pa, [pk, pk]) == 0                                      # the b pointers may alias each other
    assert call(e.ctx, None, "null", None, outputs=1, g=0) == ERR                        # groups == 0 still needs its arrays ...
    assert call(e.ctx, [None], None, [None], g=0) == 0                                   # ... but touches nothing
    torch.cuda.synchronize()
    assert bool((a == 1).all()) and bool((b == 1).all())
    assert call(e.ctx, *ok) == 0
    torch.cuda.synchronize()
    assert bool((o == 3).all())


@pytest.mark.parametrize("terms", [8, 9])
def test_graph_capture_replays_identically(terms, engine_factory):
    import torch
    e = engine_factory(64, 64, 3)
    nm, n, groups, outputs = 3, 64, 3, 4
    ha, hb = operands(e, n)
    a, b = _dev(e, ha), _dev(e, hb)
    bs = [b[o:] for o in range(outputs)]
    outs = [torch.zeros((groups, nm, n), dtype=torch.int64, device="cuda:0") for _ in range(outputs)]
    A = ha[:groups * terms].reshape(groups, terms, nm, n)
    want = [dot_ref(A, hb[o:o + terms], e.P) for o in range(outputs)]
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):                   # no warm-up is needed: the call allocates nothing
            e.dot_multi(a, (terms, 1), bs, 1, groups, terms, outs=outs)
    for _ in range(3):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for o in range(outputs):
            assert np.array_equal(e.to_host(outs[o]), want[o]), o
