"""GPU: the RNS base conversion and the mod-down by the last k moduli (include/nflhip.h "RNS base conversion",
nfllib_amd/csrc/kernels_baseconv.hip), word for word against the Python-integer restatement of tests/baseconv_util.py: no tolerance
anywhere.  The shapes are the smallest at which each path of the kernel runs: 16-byte groups and single words, the register plans
(ks <= 4, ks <= 16) and the chunked plan (ks > 16), rows past the 92nd 64-bit modulus, and a batch that wraps the grid-stride loop."""
import numpy as np
import pytest

import baseconv_util as B
from rescale_util import rescale_rns

pytestmark = pytest.mark.gpu

N = 64
# prefix to suffix, suffix to prefix, middle to all, ks = 1, kd = 1, S = D
PAIRS = {(64, 4): [((0, 2), (2, 2)), ((2, 2), (0, 2)), ((1, 2), (0, 4)), ((3, 1), (0, 4)), ((0, 3), (3, 1)), ((0, 4), (0, 4))],
         (32, 3): [((0, 2), (2, 1)), ((1, 2), (0, 1)), ((1, 1), (0, 3)), ((2, 1), (0, 3)), ((0, 2), (2, 1)), ((0, 3), (0, 3))]}
_INPUTS = {}


def inputs(e, src, seed=3):
    """batch 3: random words; the edge values of rows src planted in polynomial 0, the values around and inside the centred
    band in polynomial 1, every source word p_i - 1 and every y_i = p_i - 1 in the last two positions of polynomial 2"""
    key = (e.limb_bits, e.degree, e.nmoduli, src, seed)
    if key not in _INPUTS:
        P = e.P
        a = B.random_batch(P, e.degree, 3, e.np_dtype, seed)
        B.plant(a, P, src, B.edge_values(P, src), b=0)
        B.plant(a, P, src, B.band_values(P, src, e.limb_bits), b=1)
        s = slice(src[0], src[0] + src[1])
        a[2, s, e.degree - 1] = [p - 1 for p in P[s]]
        a[2, s, e.degree - 2] = B.all_y_max(P, src)
        a.setflags(write=False)
        _INPUTS[key] = a
    return _INPUTS[key]


def pattern(e, batch):
    """a recognisable fill for rows that must stay as they are"""
    import torch
    t = torch.arange(batch * e.words_per_poly, dtype=torch.int64, device="cuda:0") % 8191 + 1
    return t.to(e.torch_dtype).reshape(batch, e.nmoduli, e.degree)


def check_pair(e, src, dst):
    import torch
    P = e.P
    a = inputs(e, src)
    d = e.to_device(a)
    outs = {}
    for centered in (False, True):
        want = B.baseconv_rns(a, P, src, dst, centered=centered)
        # out of place: rows outside D keep the pattern
        o = pattern(e, len(a))
        keep = o.clone()
        assert e.baseconv(d, src, dst, centered=centered, out=o) is o
        rows = list(range(dst[0], dst[0] + dst[1]))
        other = [j for j in range(e.nmoduli) if j not in rows]
        assert torch.equal(o[:, rows], e.to_device(want)[:, rows]), (src, dst, centered)
        assert torch.equal(o[:, other], keep[:, other]), (src, dst, centered)
        # in place: rows outside D keep the input
        x = d.clone()
        assert e.baseconv(x, src, dst, centered=centered) is x
        assert torch.equal(x, e.to_device(want)), (src, dst, centered, "in place")
        outs[centered] = want
    assert np.array_equal(e.to_host(d), a)
    return a, outs


@pytest.mark.parametrize("lb,nm", list(PAIRS))
def test_every_pair_of_ranges_fast_and_centred(lb, nm, engine_factory):
    e = engine_factory(lb, N, nm)
    differ = 0
    for src, dst in PAIRS[(lb, nm)]:
        a, outs = check_pair(e, src, dst)
        _, u, v = B.parts(a, e.P, src)
        assert set(np.unique((v - u).astype(int)).tolist()) == {0, 1}, (src, dst)     # the planted positions reach both
        if not (src[0] <= dst[0] and dst[0] + dst[1] <= src[0] + src[1]):
            rows = slice(dst[0], dst[0] + dst[1])
            assert not np.array_equal(outs[False][:, rows], outs[True][:, rows])     # a row differs between the two modes
            differ += 1
    assert differ >= 4
    mod_up = e.mod_up(e.to_device(inputs(e, (0, 2))), (0, 2))
    assert np.array_equal(e.to_host(mod_up), B.baseconv_rns(inputs(e, (0, 2)), e.P, (0, 2), (0, nm)))


def test_band_positions_by_crt_on_the_host(engine_factory):
    """u64: random data never reaches the band.  x just below 1/2, inside the band and just above it: v - u = 0, either, 1."""
    e = engine_factory(64, N, 4)
    P, src, dst = e.P, (0, 2), (2, 2)
    vals = B.band_values(P, src, 64)
    a = B.plant(np.zeros((1, 4, N), dtype=np.uint64), P, src, vals)
    _, u, v = B.parts(a, P, src)
    d = (v - u).astype(int)[0, :len(vals)].tolist()
    assert d[:2] == [0, 0] and d[-2:] == [1, 1] and set(d) == {0, 1}
    fast = e.to_host(e.baseconv(e.to_device(a), src, dst))
    cen = e.to_host(e.baseconv(e.to_device(a), src, dst, centered=True))
    assert np.array_equal(fast, B.baseconv_rns(a, P, src, dst)) and np.array_equal(cen, B.baseconv_rns(a, P, src, dst, centered=True))
    Q = B.prod(P[:2])
    for t, (x, dx) in enumerate(zip(vals, d)):
        for j in (2, 3):
            assert int(cen[0, j, t]) == (x - dx * Q) % P[j]
    assert not np.array_equal(fast[:, 2:, :len(vals)], cen[:, 2:, :len(vals)])


def test_u16_words_and_a_misaligned_pointer(engine_factory):
    import torch
    e = engine_factory(16, 4, 2)                      # rows of 8 bytes: the word variant
    for src, dst in (((0, 1), (1, 1)), ((1, 1), (0, 2)), ((0, 2), (0, 2))):
        a = B.random_batch(e.P, 4, 3, e.np_dtype, 5)
        B.plant(a, e.P, src, B.edge_values(e.P, src)[2:], b=0)
        for centered in (False, True):
            got = e.to_host(e.baseconv(e.to_device(a), src, dst, centered=centered))
            assert np.array_equal(got, B.baseconv_rns(a, e.P, src, dst, centered=centered)), (src, dst, centered)
    assert np.array_equal(e.to_host(e.mod_down(e.to_device(a), 1)), B.moddown_rns(a, e.P, 1))
    e = engine_factory(64, N, 4)                      # a pointer one word past a 16-byte boundary
    src, dst = (1, 2), (0, 4)
    a = inputs(e, src)
    buf = torch.zeros(a.size + 1, dtype=torch.int64, device="cuda:0")
    for centered in (False, True):
        buf[1:].copy_(e.to_device(a).view(-1))
        e.baseconv(buf[1:], src, dst, centered=centered)
        assert np.array_equal(e.to_host(buf[1:]).reshape(a.shape), B.baseconv_rns(a, e.P, src, dst, centered=centered))
        assert int(buf[0]) == 0
    buf[1:].copy_(e.to_device(a).view(-1))
    out = torch.zeros(3 * 2 * N + 1, dtype=torch.int64, device="cuda:0")
    e.mod_down(buf[1:], 2, out=out[1:])
    assert np.array_equal(e.to_host(out[1:]).reshape(3, 2, N), B.moddown_rns(a, e.P, 2)) and int(out[0]) == 0


@pytest.mark.parametrize("src,dst", [((81, 15), (0, 96)), ((0, 16), (80, 16)), ((70, 17), (60, 36)), ((0, 31), (31, 2)), ((64, 32), (90, 6)),
                                     ((10, 33), (0, 50)), ((48, 48), (0, 96)), ((92, 4), (0, 8)), ((0, 4), (92, 4))])
def test_many_rows_past_the_92nd_modulus(src, dst, engine_factory):
    """u64/64/96: ks on both sides of the register plans' limits and of the 16-term chunk; the largest accumulators; source inside
    the large-delta rows (92 ..) with the destination outside, and the other way round"""
    e = engine_factory(64, N, 96)
    assert (2**62 - e.P[92]) >= 2**32 > (2**62 - e.P[91])
    check_pair(e, src, dst)


@pytest.mark.parametrize("lb,nm,k", [(64, 4, 1), (64, 4, 2), (64, 4, 3), (32, 3, 2), (64, 96, 17)])
def test_mod_down(lb, nm, k, engine_factory):
    import torch
    e = engine_factory(lb, N, nm)
    a = inputs(e, (nm - k, k), seed=6)
    d = e.to_device(a)
    for floor in (False, True):
        want = B.moddown_rns(a, e.P, k, floor=floor)
        got = e.mod_down(d, k, floor=floor)
        assert got.shape == (3, nm - k, N) and np.array_equal(e.to_host(got), want), (k, floor)
        assert np.array_equal(e.h_mod_down(a, k, floor=floor), want)
    band = B.in_band(a, e.P, (nm - k, k))
    near = B.moddown_exact(a, e.P, k, "nearest")
    got = e.to_host(e.mod_down(d, k))
    assert np.array_equal(np.where(band[:, None, :], 0, got), np.where(band[:, None, :], 0, near))
    if k == 1:
        b = np.array(a)
        b[:, nm - 1, :][band] = 0                       # an input outside the band: the mod-down by one modulus is the rescale
        assert torch.equal(e.mod_down(e.to_device(b), 1), e.rescale(e.to_device(b)))
        assert np.array_equal(e.to_host(e.rescale(e.to_device(b))), rescale_rns(b, e.P))
    assert np.array_equal(e.to_host(d), a)


def test_grid_stride_wraps_once(engine_factory):
    """u32/64/3: 16 groups per polynomial, 1024 workgroups of 256 threads -- 16400 polynomials wrap the loop once.  Sampled
    polynomials on both sides of the wrap against the restatement, every polynomial against the same call on small batches."""
    import torch
    e = engine_factory(32, N, 3)
    batch = 16400
    assert batch * N // 4 > 1024 * 256
    d = e.fill_uniform(e.empty(batch), 3, 0)
    pick = [0, 1, 16383, 16384, 16385, batch - 1]
    x = e.to_host(d[pick])
    up = e.baseconv(d.clone(), (0, 1), (0, 3), centered=True)
    down = e.mod_down(d, 2)
    assert np.array_equal(e.to_host(up[pick]), B.baseconv_rns(x, e.P, (0, 1), (0, 3), centered=True))
    assert np.array_equal(e.to_host(down[pick]), B.moddown_rns(x, e.P, 2))
    for lo in range(0, batch, 2048):
        hi = min(lo + 2048, batch)
        part = d[lo:hi].contiguous()
        assert torch.equal(down[lo:hi], e.mod_down(part, 2)), lo
        assert torch.equal(up[lo:hi], e.baseconv(part, (0, 1), (0, 3), centered=True)), lo


@pytest.mark.parametrize("lb,nm", [(64, 4), (32, 3), (16, 2), (64, 96)])
def test_compiled_variant_gives_the_same_words(lb, nm, engine_factory, compiled_engine_factory):
    import torch
    n = 4 if lb == 16 else N
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(3), 21, 0)
    k = 17 if nm == 96 else nm - 1
    for src, dst in (((0, 1), (0, nm)), ((nm - k, k), (0, nm))):
        for centered in (False, True):
            assert torch.equal(e.baseconv(d.clone(), src, dst, centered=centered), c.baseconv(d.clone(), src, dst, centered=centered))
    for floor in (False, True):
        assert torch.equal(e.mod_down(d, k, floor=floor), c.mod_down(d, k, floor=floor))


def test_host_variant_equals_device_variant(engine_factory):
    e = engine_factory(64, N, 4)
    a = inputs(e, (1, 2))
    for centered in (False, True):
        assert np.array_equal(e.h_baseconv(a, (1, 2), (0, 4), centered=centered), B.baseconv_rns(a, e.P, (1, 2), (0, 4), centered=centered))
    assert np.array_equal(e.h_baseconv(a, (3, 1), (0, 1)), B.baseconv_rns(a, e.P, (3, 1), (0, 1)))


def test_graph_capture_replays_identically(engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call (it uploads the pair's tables), then baseconv + ntt_fwd captured"""
    import torch
    e = engine_factory(64, N, 4)
    src, dst = (0, 2), (0, 4)
    a = inputs(e, src)
    want = oracle_factory(64, N, 4).ntt(B.baseconv_rns(a, e.P, src, dst, centered=True))
    x = torch.zeros((3, 4, N), dtype=torch.int64, device="cuda:0")
    d = e.to_device(a)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        e.baseconv(d, src, dst, centered=True, out=x)          # the warm-up: the first call for the pair allocates
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            e.baseconv(d, src, dst, centered=True, out=x)
            e.ntt_(x)
    for _ in range(3):
        x.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(x), want)


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    L, ERR = _lib.lib, _lib.ERR_INVALID
    e = engine_factory(64, N, 4)
    d = e.fill_uniform(e.empty(4), 1, 0)
    o = torch.zeros((8, 4, N), dtype=torch.int64, device="cuda:0")
    p, q = d.data_ptr(), o.data_ptr()
    row = N * 8
    bc, md = L.nflhip_baseconv_dev, L.nflhip_moddown_dev
    assert bc(None, q, p, 4, 0, 2, 2, 2, 0, None) == ERR                       # NULL context
    assert bc(e.ctx, None, p, 4, 0, 2, 2, 2, 0, None) == ERR                   # NULL output
    assert bc(e.ctx, q, None, 4, 0, 2, 2, 2, 0, None) == ERR                   # NULL input
    for s0, ks, d0, kd in ((0, 0, 0, 1), (0, 1, 0, 0), (4, 1, 0, 1), (3, 2, 0, 1), (0, 5, 0, 1), (0, 1, 4, 1), (0, 1, 2, 3),
                           (0, 2**63, 0, 1), (2**64 - 1, 2, 0, 1), (0, 1, 2**64 - 1, 2)):
        assert bc(e.ctx, q, p, 4, s0, ks, d0, kd, 0, None) == ERR, (s0, ks, d0, kd)   # ranges
    for flags in (1, 2, 0x200, 0x101, -1):
        assert bc(e.ctx, q, p, 4, 0, 2, 2, 2, flags, None) == ERR              # unknown flag bits
        assert md(e.ctx, q, p, 4, 1, flags, None) == ERR
    assert bc(e.ctx, p + row, p, 4, 0, 2, 2, 2, 0, None) == ERR                # an overlap that is not "the same buffer"
    assert bc(e.ctx, p - 16 * row + 8, p, 4, 0, 2, 2, 2, 0, None) == ERR       # output's last word on the input's first
    assert bc(e.ctx, q, p, 2**61, 0, 2, 2, 2, 0, None) == ERR                  # the size overflows
    for k in (0, 4, 5, 2**64 - 1):
        assert md(e.ctx, q, p, 4, k, 0, None) == ERR                           # k out of range
    assert md(e.ctx, p, p, 4, 1, 0, None) == ERR                               # mod-down in place
    assert md(e.ctx, p + row, p, 4, 1, 0, None) == ERR                         # output inside the input
    assert md(e.ctx, p - 12 * row + 8, p, 4, 1, 0, None) == ERR                # output's last word on the input's first
    assert md(e.ctx, None, p, 4, 1, 0, None) == ERR and md(e.ctx, q, None, 4, 1, 0, None) == ERR
    assert md(None, q, p, 4, 1, 0, None) == ERR
    h = e.to_host(d)
    ho = np.zeros_like(h)
    hp = h.ctypes.data
    assert L.nflhip_baseconv(e.ctx, ho.ctypes.data, hp, 4, 0, 2, 2, 3, 0) == ERR    # host: ranges
    assert L.nflhip_baseconv(e.ctx, None, hp, 4, 0, 2, 2, 2, 0) == ERR              # host: NULL
    assert L.nflhip_baseconv(e.ctx, hp + row, hp, 2, 0, 2, 2, 2, 0) == ERR          # host: overlap
    assert L.nflhip_moddown(e.ctx, hp, hp, 4, 1, 0) == ERR                          # host: in place
    assert L.nflhip_moddown(e.ctx, ho.ctypes.data, hp, 4, 4, 0) == ERR              # host: k
    assert bc(e.ctx, None, None, 0, 0, 2, 2, 2, 0, None) == 0                  # an empty batch is fine
    assert md(e.ctx, None, None, 0, 1, 0, None) == 0
    # a repeated source modulus is refused by the table builder, on the host: a context over moduli 0, 1, 0
    import ctypes as C
    from nfllib_amd.params import params
    pr = params(64)
    idx = [0, 1, 0]
    tabs = [np.ascontiguousarray(t[idx]) for t in (pr.P, pr.primitive_roots, pr.invkmax)]
    ctx = C.c_void_p()
    assert L.nflhip_ctx_create(C.byref(ctx), 0, 64, N, 3, *[t.ctypes.data_as(C.c_void_p) for t in tabs], pr.kmax_log2) == 0
    try:
        assert bc(ctx, q, p, 1, 0, 3, 0, 3, 0, None) == ERR
        assert b"source modulus repeats" in L.nflhip_last_error(ctx)
        assert md(ctx, q, p, 1, 1, 0, None) == ERR                              # the kept row 0 repeats the dropped modulus
        assert bc(ctx, q, p, 1, 0, 2, 2, 1, 0, None) == 0                       # distinct sources: served
    finally:
        L.nflhip_ctx_destroy(ctx)
    # nothing refused above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(d), h)
    o.zero_()
    assert bc(e.ctx, q, p, 4, 0, 2, 2, 2, 0, None) == 0
    want = B.baseconv_rns(h, e.P, (0, 2), (2, 2))
    assert np.array_equal(e.to_host(o[:4])[:, 2:], want[:, 2:]) and not o[:4, :2].any() and not o[4:].any()
