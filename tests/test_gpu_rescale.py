"""GPU: the RNS rescale by the last modulus (include/nflhip.h "RNS rescale", nfllib_amd/csrc/kernels_rescale.hip), bit-exact
against the Python-integer restatements of tests/rescale_util.py: the coefficient form against the row formula on whole
rows and against the exact (CRT, divide, round) formula; the NTT form against the CPU oracle's transforms around the row
formula.  Sampled shapes: with 30 moduli at n >= 8192 and at u64/1024/94 the exact formula is checked on 64 sampled positions
per polynomial (plus the first and last); the row formula is checked on whole rows everywhere.  At batch 16384 eight sampled
polynomials are checked against the formulas and every polynomial against the same call on small batches."""
import os
import subprocess

import numpy as np
import pytest

from rescale_util import edge_batch, random_batch, rescale_exact, rescale_ntt, rescale_rns

pytestmark = pytest.mark.gpu


def _positions(n, seed):
    rnd = np.random.RandomState(seed)
    return np.unique(np.concatenate([[0, n - 1], rnd.randint(0, n, size=64)]))


def _inputs(e, n, nm, big):
    """random polynomials with the edge polynomials planted behind them (the two uniform ones alone at the largest shapes)"""
    P = e.P
    return np.concatenate([random_batch(P, n, 1 if big else 3, e.np_dtype, 11 + nm), edge_batch(P, n, e.np_dtype, combos=not big)])


def _check(e, x, big, small, sampled):
    P, n = e.P, e.degree
    want = rescale_rns(x, P)
    if sampled:
        pos = _positions(n, 5)
        assert np.array_equal(rescale_exact(x, P, pos), want[..., pos])
    else:
        assert np.array_equal(rescale_exact(x, P), want)
    got = e.to_host(e.rescale(e.to_device(x)))
    assert got.shape == want.shape and np.array_equal(got, want), "coefficient form"
    X = big.ntt(x)
    want_n = small.ntt(want)
    assert np.array_equal(e.to_host(e.rescale(e.to_device(X), ntt=True)), want_n), "NTT form"
    assert np.array_equal(e.to_host(e.rescale(e.to_device(X), ntt=True, composed=True)), want_n), "NTT form, composed plan"
    if 2 * n * e.np_dtype.itemsize <= 65536:
        assert np.array_equal(e.to_host(e.rescale(e.to_device(X), ntt=True, fused=True)), want_n), "NTT form, one-launch kernel"
    else:
        with pytest.raises(Exception, match="one-launch"):
            e.rescale(e.to_device(X), ntt=True, fused=True)
    assert np.array_equal(rescale_ntt(X, P, big, small), want_n)


@pytest.mark.parametrize("n", [4, 1024, 4096, 8192, 16384, 65536])
@pytest.mark.parametrize("nm", [2, 4, 30])
def test_u64_degrees_and_moduli(n, nm, engine_factory, oracle_factory):
    e = engine_factory(64, n, nm)
    big = n >= 8192 and nm == 30
    _check(e, _inputs(e, n, nm, big), oracle_factory(64, n, nm), oracle_factory(64, n, nm - 1), sampled=big)


@pytest.mark.parametrize("lb,n,nm", [(64, 1024, 94), (32, 1024, 2), (32, 4096, 3), (16, 128, 2), (32, 4, 2)])
def test_other_limbs_and_moduli_past_the_92nd(lb, n, nm, engine_factory, oracle_factory):
    e = engine_factory(lb, n, nm)
    _check(e, _inputs(e, n, nm, False), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - 1), sampled=nm == 94)


def test_all_words_p_minus_one_round_to_zero(engine_factory):
    e = engine_factory(64, 4096, 4)
    x = edge_batch(e.P, 4096, e.np_dtype, combos=False)
    for ntt in (False, True):
        d = e.to_device(x)
        if ntt:
            e.ntt_(d)
        got = e.to_host(e.rescale(d, ntt=ntt))
        assert not got.any()        # X = 0 and X = Q - 1 both give 0 (whose transform is 0)


@pytest.mark.parametrize("batch", [1, 3, 16384])
def test_batches_u64_4096_4(batch, engine_factory, oracle_factory):
    import torch
    e = engine_factory(64, 4096, 4)
    big, small = oracle_factory(64, 4096, 4), oracle_factory(64, 4096, 3)
    d = e.fill_uniform(e.empty(batch), 3, 0)
    pick = sorted({0, batch - 1} | set(np.random.RandomState(batch).randint(0, batch, size=6).tolist()))
    x = e.to_host(d[pick])
    want = rescale_rns(x, e.P)
    assert np.array_equal(rescale_exact(x, e.P), want)
    out = e.rescale(d)
    assert np.array_equal(e.to_host(out[pick]), want)
    D = e.ntt_(d.clone())
    out_n = e.rescale(D, ntt=True)
    assert np.array_equal(e.to_host(out_n[pick]), small.ntt(want))
    assert np.array_equal(e.to_host(e.rescale(D, ntt=True, composed=True)[pick]), small.ntt(want))
    assert torch.equal(e.rescale(D, ntt=True, fused=True), out_n)
    # every polynomial: the same call on batches of 64 (device-side comparison)
    for o, src, ntt in ((out, d, False), (out_n, D, True)):
        for lo in range(0, batch, max(batch // 4, 1)):
            hi = min(lo + 64, batch)
            assert torch.equal(o[lo:hi], e.rescale(src[lo:hi].contiguous(), ntt=ntt)), (lo, ntt)


def test_misaligned_operands_take_the_word_path(engine_factory, oracle_factory):
    """pointers that are not 16-byte aligned (an offset view of a larger buffer) are served word by word"""
    import torch
    e = engine_factory(64, 1024, 2)
    x = _inputs(e, 1024, 2, False)
    b = len(x)
    src = torch.zeros(x.size + 1, dtype=torch.int64, device="cuda:0")
    dst = torch.zeros(b * 1024 + 1, dtype=torch.int64, device="cuda:0")
    want = rescale_rns(x, e.P)
    src[1:].copy_(e.to_device(x).view(-1))
    e.rescale(src[1:], out=dst[1:])
    assert np.array_equal(e.to_host(dst[1:]).reshape(want.shape), want)
    src[1:].copy_(e.to_device(oracle_factory(64, 1024, 2).ntt(x)).view(-1))
    for plan in ({}, {"composed": True}, {"fused": True}):
        dst.zero_()
        e.rescale(src[1:], ntt=True, out=dst[1:], **plan)
        assert np.array_equal(e.to_host(dst[1:]).reshape(want.shape), oracle_factory(64, 1024, 1).ntt(want)), plan


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (64, 65536, 2), (64, 8192, 3), (32, 1024, 2), (32, 8192, 2), (16, 128, 2), (64, 1024, 94)])
def test_forms_commute_with_the_device_transforms(lb, n, nm, engine_factory):
    """intt'(rescale(ntt(x), ntt=True)) == rescale(x) and ntt'(rescale(x)) == rescale(ntt(x), ntt=True), ' = the smaller context"""
    e, s = engine_factory(lb, n, nm), engine_factory(lb, n, nm - 1)
    x = e.fill_uniform(e.empty(3), 4, 0)
    X = e.ntt_(x.clone())
    y = e.rescale(x)
    Y = e.rescale(X, ntt=True)
    assert np.array_equal(s.to_host(s.ntt_(y.clone())), s.to_host(Y))
    assert np.array_equal(s.to_host(s.intt_(Y.clone())), s.to_host(y))


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (64, 1024, 2), (64, 16384, 2), (32, 1024, 2), (32, 4096, 3), (16, 128, 2), (64, 1024, 94)])
def test_compiled_variant_equals_default(lb, n, nm, engine_factory, compiled_engine_factory):
    """a context created under NFLHIP_VARIANT=hipcc composes the NTT form from the compiled transforms: the independent
    cross-check of the one-launch kernel (and of the generated transforms inside the default composed plan)"""
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    x = e.fill_uniform(e.empty(5), 21, 0)
    X = e.ntt_(x.clone())
    assert np.array_equal(e.to_host(e.rescale(x)), c.to_host(c.rescale(x)))
    want = e.to_host(e.rescale(X, ntt=True))
    assert np.array_equal(want, c.to_host(c.rescale(X, ntt=True)))
    assert np.array_equal(want, e.to_host(e.rescale(X, ntt=True, composed=True)))
    if 2 * n * e.np_dtype.itemsize <= 65536:
        assert np.array_equal(want, e.to_host(e.rescale(X, ntt=True, fused=True)))
        assert np.array_equal(want, c.to_host(c.rescale(X, ntt=True, fused=True)))


@pytest.mark.parametrize("lb", [64, 32])
def test_chain_4_3_2_1(lb, engine_factory):
    n = 1024
    es = {nm: engine_factory(lb, n, nm) for nm in (4, 3, 2, 1)}
    x = np.concatenate([random_batch(es[4].P, n, 2, es[4].np_dtype, 2), edge_batch(es[4].P, n, es[4].np_dtype)])
    want, d = x, es[4].to_device(x)
    D = es[4].ntt_(d.clone())
    for nm in (4, 3, 2):
        want = rescale_exact(want, es[nm].P)
        d = es[nm].rescale(d)
        D = es[nm].rescale(D, ntt=True)
        assert np.array_equal(es[nm - 1].to_host(d), want), nm
    assert want.shape == (len(x), 1, n)
    assert np.array_equal(es[1].to_host(es[1].intt_(D)), want)


@pytest.mark.parametrize("lb,n,nm,batch", [(64, 4096, 4, 3), (64, 4096, 4, 300), (32, 1024, 2, 5), (16, 128, 2, 2)])
def test_host_variant_equals_device_variant(lb, n, nm, batch, engine_factory):
    e = engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(batch), 8, 0)
    h = e.to_host(d)
    assert np.array_equal(e.h_rescale(h), e.to_host(e.rescale(d)))
    D = e.ntt_(d.clone())
    assert np.array_equal(e.h_rescale(e.to_host(D), ntt=True), e.to_host(e.rescale(D, ntt=True)))


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    L, ERR = _lib.lib, _lib.ERR_INVALID
    e = engine_factory(64, 1024, 2)
    d = e.fill_uniform(e.empty(4), 1, 0)
    o = torch.zeros((8, 1, 1024), dtype=torch.int64, device="cuda:0")
    p, q = d.data_ptr(), o.data_ptr()
    row = 1024 * 8
    assert L.nflhip_rescale_dev(None, q, p, 4, 0, None) == ERR                    # NULL context
    assert L.nflhip_rescale_dev(e.ctx, None, p, 4, 0, None) == ERR                # NULL output
    assert L.nflhip_rescale_dev(e.ctx, q, None, 4, 1, None) == ERR                # NULL input
    for form in (2, -1, 0x100, 0x102, 0x200, 0x301, 0x401):
        assert L.nflhip_rescale_dev(e.ctx, q, p, 4, form, None) == ERR            # unknown form
    assert L.nflhip_rescale_dev(e.ctx, p, p, 4, 0, None) == ERR                   # in place
    assert L.nflhip_rescale_dev(e.ctx, p + row, p, 4, 1, None) == ERR             # output inside the input
    assert L.nflhip_rescale_dev(e.ctx, p - 4 * row + 8, p, 4, 0, None) == ERR     # output's last word on the input's first
    assert L.nflhip_rescale_dev(e.ctx, p, p - 2 * row + 8, 1, 0, None) == ERR     # input's last word on the output's first
    one = engine_factory(64, 1024, 1)
    assert L.nflhip_rescale_dev(one.ctx, q, p, 1, 0, None) == ERR                 # a single modulus
    assert L.nflhip_rescale(one.ctx, q, p, 1, 0) == ERR
    h = e.to_host(d)
    ho = np.zeros((4, 1, 1024), dtype=np.uint64)
    hp = h.ctypes.data
    assert L.nflhip_rescale(e.ctx, ho.ctypes.data, hp, 4, 7) == ERR               # host: unknown form
    assert L.nflhip_rescale(e.ctx, None, hp, 4, 0) == ERR                         # host: NULL
    assert L.nflhip_rescale(e.ctx, hp, hp, 4, 0) == ERR                           # host: in place
    assert L.nflhip_rescale(e.ctx, hp + row, hp, 2, 1) == ERR                     # host: overlap
    assert L.nflhip_rescale_dev(e.ctx, None, None, 0, 0, None) == 0               # an empty batch is fine
    # nothing above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(d), h) and not o.any()
    assert L.nflhip_rescale_dev(e.ctx, q, p, 4, 0, None) == 0                     # adjacent buffers, valid call
    assert np.array_equal(e.to_host(o[:4]), rescale_rns(h, e.P))


def test_graph_capture_replays_identically(engine_factory, oracle_factory):
    """the one-launch NTT-form call (and the coefficient form) at u64/4096/4: no scratch, no allocation, capturable"""
    import torch
    e = engine_factory(64, 4096, 4)
    a = e.fill_uniform(e.empty(4), 6, 0)
    A = e.ntt_(a.clone())
    want = rescale_rns(e.to_host(a), e.P)
    want_n = oracle_factory(64, 4096, 3).ntt(want)
    x = torch.zeros((4, 3, 4096), dtype=torch.int64, device="cuda:0")
    y = torch.zeros_like(x)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        e.rescale(a, out=x)
        e.rescale(A, ntt=True, out=y, fused=True)
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            e.rescale(a, out=x)
            e.rescale(A, ntt=True, out=y, fused=True)
    for _ in range(3):
        x.zero_()
        y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(x), want)
        assert np.array_equal(e.to_host(y), want_n)


@pytest.mark.parametrize("compiled,n,nm", [(True, 64, 3), (False, 4096, 2)])
def test_two_streams_share_the_composed_plans_scratch(compiled, n, nm, engine_factory, compiled_engine_factory, oracle_factory):
    """the NTT form's default plan composes on both contexts -- a compiled one at any degree, a default one from rows of 32 KiB on --
    so calls alternating between two streams share the one scratch and its event"""
    import torch
    e = (compiled_engine_factory if compiled else engine_factory)(64, n, nm)
    big, small = oracle_factory(64, n, nm), oracle_factory(64, n, nm - 1)
    a, b = random_batch(e.P, n, 2, e.np_dtype, 31), random_batch(e.P, n, 2, e.np_dtype, 32)
    wa, wb = small.ntt(rescale_rns(a, e.P)), small.ntt(rescale_rns(b, e.P))
    dA, dB = e.to_device(big.ntt(a)), e.to_device(big.ntt(b))
    ya = torch.zeros((2, nm - 1, n), dtype=torch.int64, device="cuda:0")
    yb = torch.zeros_like(ya)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        e.rescale(dA, ntt=True, out=ya, stream=s1)
        e.rescale(dB, ntt=True, out=yb, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(ya), wa) and np.array_equal(e.to_host(yb), wb)


def test_first_composed_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import ctypes as C
    import torch
    from nfllib_amd import Engine, _lib
    saved = os.environ.get("NFLHIP_VARIANT")
    os.environ["NFLHIP_VARIANT"] = "hipcc"
    try:
        e = Engine(64, 64, 3, device=0)                        # a context of its own: no child context, no scratch yet
    finally:
        if saved is None:
            os.environ.pop("NFLHIP_VARIANT", None)
        else:
            os.environ["NFLHIP_VARIANT"] = saved
    try:
        a = random_batch(e.P, 64, 2, e.np_dtype, 33)
        want = oracle_factory(64, 64, 2).ntt(rescale_rns(a, e.P))
        dA = e.to_device(oracle_factory(64, 64, 3).ntt(a))
        y = torch.full((2, 2, 64), 7, dtype=torch.int64, device="cuda:0")
        z = torch.zeros(4, device="cuda:0")
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        resc = _lib.lib.nflhip_rescale_dev
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st):
                z.add_(1)
                rc = resc(e.ctx, y.data_ptr(), dA.data_ptr(), 2, _lib.FORM_NTT, sp)
        torch.cuda.synchronize()
        assert rc == _lib.ERR_UNSUPPORTED
        assert (e.to_host(y) == 7).all()                       # nothing was enqueued
        assert resc(e.ctx, y.data_ptr(), dA.data_ptr(), 2, _lib.FORM_NTT, sp) == 0      # the same stream, after the capture
        st.synchronize()
        assert np.array_equal(e.to_host(y), want)
    finally:
        e.close()


@pytest.fixture(scope="module")
def cpp_programs(tmp_path_factory):
    from test_rescale_cpu import build_cpp
    out = str(tmp_path_factory.mktemp("cpp_rescale"))
    return build_cpp(out), build_cpp(out, eager=True)


@pytest.mark.parametrize("mode", ["thread0", "thread1", "eager_runtime", "eager_build"])
def test_cpp_surface_on_the_gpu(mode, cpp_programs):
    """poly, poly_p (deferred operations pending on both ring types, before and after), device_batch, a one-device
    sharded_batch -- under both queue executors and with deferred execution off"""
    exe = cpp_programs[1] if mode == "eager_build" else cpp_programs[0]
    env = dict(os.environ)
    env["NFL_HIP_QUEUE_THREAD"] = "0" if mode == "thread0" else "1"
    args = [exe] + (["eager"] if mode == "eager_runtime" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
