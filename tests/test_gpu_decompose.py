"""GPU: the gadget decomposition (include/nflhip.h "gadget decomposition", nfllib_amd/csrc/kernels_decompose.hip), bit for bit
against the Python-integer restatement of tests/decompose_util.py: words and compact output, both digit modes, gadget_mul, the
NTT form under both plans, the key-switching identity through nflhip_dot_dev, one noise-free key switch, the argument checks, graph
capture and the C++ surface.  Every comparison is equality of words.

Widths per shape: every w of {1, 7, 8, 15, 16, 20, 31, bits - 1} that the limb width allows on the short rows (where l is large the
output stays small); two or three of them on the rows of 1024 and 4096 words."""
import os
import subprocess

import numpy as np
import pytest

from decompose_util import decompose_ref, edge_batch, gadget_mul_ref, nbits, ndigits

pytestmark = pytest.mark.gpu

ALL_W = (1, 7, 8, 15, 16, 20, 31)
_CMAX = {"i8": 7, "i16": 15, "i32": 31}


def widths(lb, n, nm):
    bits = nbits(lb)
    if n <= 128:
        ws = [w for w in ALL_W if w <= bits - 1] + [bits - 1]
    elif n == 1024:
        ws = ([1, 7] if nm == 1 else []) + [15 if nm == 2 else 8, 20, 31, bits - 1]
    else:
        ws = [16, 31, bits - 1]
    return sorted({w for w in ws if w <= bits - 1})


def row_bytes(e):
    return e.degree * e.np_dtype.itemsize


def ntt_plans(e):
    return [None, "composed"] + (["fused"] if row_bytes(e) <= 32768 else [])


def check_shape(e, w, batch, seed):
    """words (both modes) against the restatement; compact formats against it and, expanded, against the words; gadget_mul; the
    NTT form under every plan against the device's forward transform of the coefficient form"""
    import torch
    lb, n, P = e.limb_bits, e.degree, e.P
    x = edge_batch(P, n, lb, w, batch, seed)
    d = e.to_device(x)
    terms = e.decompose_terms(w)
    assert terms == len(P) * ndigits(lb, w)
    for signed in (False, True):
        want = decompose_ref(x, P, lb, w, signed)
        words = e.decompose(d, w, signed=signed)
        assert tuple(words.shape) == (len(x) * terms, len(P), n)
        assert np.array_equal(e.to_host(words), want), (w, signed)
        for fmt, wmax in _CMAX.items():
            if w > wmax:
                continue
            c = e.decompose(d, w, signed=signed, fmt=fmt)
            assert tuple(c.shape) == (len(x) * terms, n)
            assert np.array_equal(c.cpu().numpy(), decompose_ref(x, P, lb, w, signed, fmt)), (w, signed, fmt)
            assert torch.equal(e.expand_small(c), words), (w, signed, fmt)
        want_n = e.ntt_(words.clone())
        for plan in ntt_plans(e):
            assert torch.equal(e.decompose(d, w, signed=signed, ntt=True, plan=plan), want_n), (w, signed, plan)
    assert np.array_equal(e.to_host(e.gadget_mul(d, w)), gadget_mul_ref(x, P, lb, w)), w
    return x, d


SHAPES = [(64, n, nm) for n in (4, 1024, 4096) for nm in (1, 2, 4)] + [(32, 4096, 3), (32, 4, 2), (16, 128, 2), (16, 4, 1)]


@pytest.mark.parametrize("lb,n,nm", SHAPES)
def test_shapes_widths_and_modes(lb, n, nm, engine_factory):
    e = engine_factory(lb, n, nm)
    for k, w in enumerate(widths(lb, n, nm)):
        check_shape(e, w, 3 if k % 2 == 0 else 1, 17 * k + nm)


def test_rows_past_the_92nd_modulus(engine_factory):
    """(64, 64, 96) at w = 31: the forward transforms of the last rows are another kernel family"""
    check_shape(engine_factory(64, 64, 96), 31, 1, 5)


@pytest.mark.parametrize("lb,n,nm,w", [(64, 8192, 2, 31), (32, 16384, 2, 20)])
def test_fused_plan_is_unsupported_beyond_32_kib_rows(lb, n, nm, w, engine_factory):
    import torch
    from nfllib_amd import NflHipError, _lib
    e = engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(2), 3, 0)
    with pytest.raises(NflHipError) as ei:
        e.decompose(d, w, ntt=True, plan="fused")
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    words = e.decompose(d, w, signed=True)
    assert np.array_equal(e.to_host(words), decompose_ref(e.to_host(d), e.P, lb, w, True))
    want_n = e.ntt_(words.clone())
    assert torch.equal(e.decompose(d, w, signed=True, ntt=True), want_n)                     # the default takes the composed plan
    assert torch.equal(e.decompose(d, w, signed=True, ntt=True, plan="composed"), want_n)


@pytest.mark.parametrize("lb,n,nm,w", [(64, 4096, 4, 31), (64, 1024, 2, 20), (32, 1024, 2, 15), (32, 4096, 3, 8), (16, 128, 2, 7), (64, 64, 96, 31)])
def test_compiled_variant_equals_default(lb, n, nm, w, engine_factory, compiled_engine_factory):
    """a context created under NFLHIP_VARIANT=hipcc takes the composed plan over the compiled transforms: the independent
    cross-check of the one-launch kernel"""
    import torch
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    d = e.to_device(edge_batch(e.P, n, lb, w, 2, 4))
    for signed in (False, True):
        assert torch.equal(e.decompose(d, w, signed=signed), c.decompose(d, w, signed=signed))
        want = e.decompose(d, w, signed=signed, ntt=True)
        assert torch.equal(want, c.decompose(d, w, signed=signed, ntt=True))
        assert torch.equal(want, c.decompose(d, w, signed=signed, ntt=True, plan="fused"))
    assert torch.equal(e.gadget_mul(d, w), c.gadget_mul(d, w))


@pytest.mark.parametrize("lb,n,nm,w,batch", [(64, 4096, 4, 31, 3), (64, 1024, 2, 7, 40), (32, 1024, 2, 15, 5), (16, 128, 2, 7, 2)])
def test_host_variant_equals_device_variant(lb, n, nm, w, batch, engine_factory):
    e = engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(batch), 8, 0)
    h = e.to_host(d)
    assert np.array_equal(e.h_decompose(h, w, signed=True), e.to_host(e.decompose(d, w, signed=True)))
    assert np.array_equal(e.h_decompose(h, w, ntt=True), e.to_host(e.decompose(d, w, ntt=True)))
    fmt = "i8" if w <= 7 else "i16" if w <= 15 else "i32"
    assert np.array_equal(e.h_decompose(h, w, signed=True, fmt=fmt), e.decompose(d, w, signed=True, fmt=fmt).cpu().numpy())


@pytest.mark.parametrize("lb,n,nm,w", [(64, 1024, 2, 20), (32, 1024, 2, 7), (16, 128, 2, 7)])
def test_misaligned_operands_take_the_word_path(lb, n, nm, w, engine_factory):
    """input and output offset by one word (an offset view of a larger buffer): served word by word, same words"""
    import torch
    e = engine_factory(lb, n, nm)
    x = edge_batch(e.P, n, lb, w, 2, 9)
    terms, words = e.decompose_terms(w), x.size
    src = torch.zeros(words + 1, dtype=e.torch_dtype, device="cuda:0")
    src[1:].copy_(e.to_device(x).view(-1))
    dst = torch.zeros(words * terms + 1, dtype=e.torch_dtype, device="cuda:0")
    shape = (len(x) * terms, nm, n)
    for signed in (False, True):
        want = decompose_ref(x, e.P, lb, w, signed)
        dst.zero_()
        e.decompose(src[1:], w, signed=signed, out=dst[1:])
        assert np.array_equal(e.to_host(dst[1:]).reshape(shape), want) and int(dst[0]) == 0
        want_n = e.to_host(e.ntt_(e.to_device(want)))
        for plan in (None, "fused") + (("composed",) if lb == 64 else ()):   # (the composed plan hands the pointer to the transform launchers)
            dst.zero_()
            e.decompose(src[1:], w, signed=signed, ntt=True, out=dst[1:], plan=plan)
            assert np.array_equal(e.to_host(dst[1:]).reshape(shape), want_n), plan
        fmt, tdt = ("i8", torch.int8) if w <= 7 else ("i32", torch.int32)
        cd = torch.zeros(len(x) * terms * n + 1, dtype=tdt, device="cuda:0")
        e.decompose(src[1:], w, signed=signed, fmt=fmt, out=cd[1:])
        assert np.array_equal(cd[1:].cpu().numpy().reshape(len(x) * terms, n), decompose_ref(x, e.P, lb, w, signed, fmt)) and int(cd[0]) == 0
    dst.zero_()
    e.gadget_mul(src[1:], w, out=dst[1:])
    assert np.array_equal(e.to_host(dst[1:]).reshape(shape), gadget_mul_ref(x, e.P, lb, w))


@pytest.mark.parametrize("lb,n,nm,w,signed", [(64, 4096, 4, 31, False), (64, 1024, 2, 20, True), (32, 1024, 2, 15, False), (16, 128, 2, 7, True)])
def test_decompose_dot_gadget_equals_polymul(lb, n, nm, w, signed, engine_factory):
    """ntt_inv(dot(decompose(x, NTT), ntt_fwd(gadget_mul(y)), terms)) == polymul(x, y), bit for bit"""
    import torch
    e = engine_factory(lb, n, nm)
    batch = 3
    x = e.to_device(edge_batch(e.P, n, lb, w, batch, 21)[:batch])
    y = e.fill_uniform(e.empty(batch), 5, 1)
    terms = e.decompose_terms(w)
    D = e.decompose(x, w, signed=signed, ntt=True)
    G = e.ntt_(e.gadget_mul(y, w))
    got = e.intt_(e.dot(D, G, terms))
    assert torch.equal(got, e.polymul(x, y))


@pytest.mark.parametrize("lb,n,nm,w", [(64, 1024, 2, 20), (32, 1024, 2, 15)])
def test_one_noise_free_key_switch(lb, n, nm, w, engine_factory):
    """key K_j = (a_j, a_j s + G_j(s')) with uniform a_j, laid out [term][component]; both components of the switched ciphertext
    come from nflhip_dot_dev with {K + c, 0, 2}; c_1 - c_0 s == x s' exactly"""
    import torch
    from nfllib_amd import _lib
    e = engine_factory(lb, n, nm)
    terms, batch = e.decompose_terms(w), 3
    s = e.ntt_(e.fill_uniform(e.empty(1), 31, 0))
    s2 = e.fill_uniform(e.empty(1), 32, 0)
    x = e.fill_uniform(e.empty(batch), 33, 0)
    a = e.fill_uniform(e.empty(terms), 34, 0)                         # taken as NTT-form values
    G = e.ntt_(e.gadget_mul(s2, w))
    kb = e.pointwise(_lib.OP_ADD, e.pointwise(_lib.OP_MUL, a, s.expand(terms, nm, n).contiguous()), G)
    K = torch.stack([a, kb], dim=1).contiguous()                      # [terms][2][nm][n]
    D = e.decompose(x, w, signed=True, ntt=True)
    c = [e.dot_strided(D, (terms, 1), K.data_ptr() + comp * e.bytes_per_poly, (0, 2), batch, terms) for comp in (0, 1)]
    diff = e.pointwise(_lib.OP_SUB, c[1], e.pointwise(_lib.OP_MUL, c[0], s.expand(batch, nm, n).contiguous()))
    assert torch.equal(e.intt_(diff), e.polymul(x, s2.expand(batch, nm, n).contiguous()))


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    L, ERR = _lib.lib, _lib.ERR_INVALID
    S, CO, FU = _lib.DECOMP_SIGNED, _lib.DECOMP_COMPOSED, _lib.DECOMP_FUSED
    e = engine_factory(64, 1024, 2)
    w, batch = 31, 2
    terms = e.decompose_terms(w)
    d = e.fill_uniform(e.empty(batch), 1, 0)
    o = torch.zeros((batch * terms, 2, 1024), dtype=torch.int64, device="cuda:0")
    p, q = d.data_ptr(), o.data_ptr()
    poly = e.bytes_per_poly
    assert L.nflhip_decompose_terms(e.ctx, w) == terms == 4 and L.nflhip_decompose_terms(e.ctx, 1) == 124
    for bad_w in (0, -1, 62, 63, 64, 1 << 20):
        assert L.nflhip_decompose_terms(e.ctx, bad_w) == 0
        assert L.nflhip_decompose_dev(e.ctx, q, 0, p, batch, bad_w, 0, None) == ERR       # w outside 1 .. bits - 1
        assert L.nflhip_gadget_mul_dev(e.ctx, q, p, batch, bad_w, None) == ERR
    assert L.nflhip_decompose_dev(None, q, 0, p, batch, w, 0, None) == ERR                # NULL context
    assert L.nflhip_decompose_dev(e.ctx, None, 0, p, batch, w, 0, None) == ERR            # NULL output
    assert L.nflhip_decompose_dev(e.ctx, q, 0, None, batch, w, 0, None) == ERR            # NULL input
    assert L.nflhip_gadget_mul_dev(None, q, p, batch, w, None) == ERR
    assert L.nflhip_gadget_mul_dev(e.ctx, None, p, batch, w, None) == ERR
    assert L.nflhip_gadget_mul_dev(e.ctx, q, None, batch, w, None) == ERR
    for fmt, bad_w in ((_lib.FMT_I8, 8), (_lib.FMT_I16, 16), (_lib.FMT_I32, 32)):          # compact limits
        assert L.nflhip_decompose_dev(e.ctx, q, fmt, p, batch, bad_w, 0, None) == ERR
        assert L.nflhip_decompose_dev(e.ctx, q, fmt, p, batch, bad_w, S, None) == ERR
        assert L.nflhip_decompose_dev(e.ctx, q, fmt, p, batch, bad_w - 1, 1, None) == ERR  # the NTT form with a compact format
    for fmt in (4, -1, 17):
        assert L.nflhip_decompose_dev(e.ctx, q, fmt, p, batch, w, 0, None) == ERR         # unknown format
    for flags in (2, 3, 0x800, 0x1000 | 1, -1, CO | FU | 1, CO, FU, CO | S, FU | S):         # unknown bits; both plans; a plan without the NTT form
        assert L.nflhip_decompose_dev(e.ctx, q, 0, p, batch, w, flags, None) == ERR, hex(flags)
    assert L.nflhip_decompose_dev(e.ctx, p, 0, p, batch, w, 0, None) == ERR               # in place
    assert L.nflhip_decompose_dev(e.ctx, p + poly, 0, p, batch, w, 0, None) == ERR        # output inside the input
    assert L.nflhip_decompose_dev(e.ctx, p - batch * terms * poly + 8, 0, p, batch, w, 0, None) == ERR   # output's last word on the input's first
    assert L.nflhip_decompose_dev(e.ctx, q, 0, q + batch * terms * poly - 8, batch, w, 0, None) == ERR    # input's first word on the output's last
    assert L.nflhip_gadget_mul_dev(e.ctx, p + 8, p, batch, w, None) == ERR
    assert L.nflhip_decompose_dev(e.ctx, q, 0, p, (1 << 63) // 1024, w, 0, None) == ERR   # a size that overflows size_t
    h = e.to_host(d)
    ho = np.zeros((batch * terms, 2, 1024), dtype=np.uint64)
    hp = h.ctypes.data
    assert L.nflhip_decompose(e.ctx, ho.ctypes.data, 0, hp, batch, 0, 0) == ERR           # host: w
    assert L.nflhip_decompose(e.ctx, None, 0, hp, batch, w, 0) == ERR                     # host: NULL
    assert L.nflhip_decompose(e.ctx, hp, 0, hp, batch, w, 0) == ERR                       # host: in place
    assert L.nflhip_decompose(e.ctx, ho.ctypes.data, 1, hp, batch, w, 0) == ERR           # host: int8 at w = 31
    assert L.nflhip_decompose_dev(e.ctx, None, 0, None, 0, w, 0, None) == 0               # an empty batch is fine
    assert L.nflhip_gadget_mul_dev(e.ctx, None, None, 0, w, None) == 0
    assert L.nflhip_decompose(e.ctx, None, 0, None, 0, w, 1) == 0
    # nothing above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(d), h) and not o.any() and not ho.any()
    assert L.nflhip_decompose_dev(e.ctx, q, 0, p, batch, w, S, None) == 0
    assert np.array_equal(e.to_host(o), decompose_ref(h, e.P, 64, w, True))


def test_unsupported_and_batch_zero_through_the_engine(engine_factory):
    e = engine_factory(64, 1024, 2)
    empty = e.empty(0)
    assert tuple(e.decompose(empty, 20).shape) == (0, 2, 1024)
    assert tuple(e.gadget_mul(empty, 20).shape) == (0, 2, 1024)
    with pytest.raises(ValueError):
        e.decompose(e.empty(1), 62)


def test_graph_capture_replays_on_changed_input(engine_factory):
    """the coefficient form, the one-launch NTT-form plan and gadget_mul: no scratch, no allocation, capturable; a replay on
    changed input matches a fresh call"""
    import torch
    e = engine_factory(64, 4096, 4)
    w, batch = 31, 2
    terms = e.decompose_terms(w)
    a = e.fill_uniform(e.empty(batch), 6, 0)
    x, y, z = (torch.zeros((batch * terms, 4, 4096), dtype=torch.int64, device="cuda:0") for _ in range(3))
    c = torch.zeros((batch * terms, 4096), dtype=torch.int32, device="cuda:0")

    def work():
        e.decompose(a, w, signed=True, out=x)
        e.decompose(a, w, signed=True, ntt=True, plan="fused", out=y)
        e.gadget_mul(a, w, out=z)
        e.decompose(a, w, fmt="i32", out=c)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        work()
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            work()
    for seed in (7, 8):
        e.fill_uniform(a, seed, 0)
        for t in (x, y, z, c):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fresh = e.decompose(a, w, signed=True)
        assert np.array_equal(e.to_host(fresh), decompose_ref(e.to_host(a), e.P, 64, w, True))
        assert torch.equal(x, fresh)
        assert torch.equal(y, e.ntt_(fresh.clone()))
        assert torch.equal(z, e.gadget_mul(a, w))
        assert torch.equal(c, e.decompose(a, w, fmt="i32"))


@pytest.fixture(scope="module")
def cpp_programs(tmp_path_factory):
    from test_decompose_cpu import build_cpp
    out = str(tmp_path_factory.mktemp("cpp_decompose"))
    return build_cpp(out), build_cpp(out, eager=True)


@pytest.mark.parametrize("mode", ["thread0", "thread1", "eager_runtime", "eager_build"])
def test_cpp_surface_on_the_gpu(mode, cpp_programs):
    """poly, poly_p (deferred operations pending before the call and recorded after it, outputs shared copy-on-write),
    device_batch::assign_decompose / assign_gadget_mul and the identity through nfl::dot -- under both queue executors and with
    deferred execution off"""
    exe = cpp_programs[1] if mode == "eager_build" else cpp_programs[0]
    env = dict(os.environ)
    env["NFL_HIP_QUEUE_THREAD"] = "0" if mode == "thread0" else "1"
    args = [exe] + (["eager"] if mode == "eager_runtime" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
