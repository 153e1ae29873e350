"""GPU: the Galois automorphisms sigma_k (include/nflhip.h "Galois automorphisms", nfllib_amd/csrc/kernels_automorph.hip),
bit-exact against the numpy restatement of both maps (tests/automorph_util.py) and the CPU oracle: every degree plan
(multi-row tiles, one-row tiles, NTT chunks, the L2 plan of long coefficient rows), the three limb widths, moduli past the
92nd, batch sizes, the multi form, the host-pointer variant, argument checks, graph capture, the ring homomorphism on the
device, and the header surface's C++ program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from automorph_util import sigma_coeff, sigma_ntt

pytestmark = pytest.mark.gpu


def _ks(n, seed):
    rnd = np.random.RandomState(seed)
    return [1, 3, 5, 2 * n - 1, int(rnd.randint(0, n)) * 2 + 1, 2 * n + 7]


def _check(e, d, n, seed):
    h = e.to_host(d)
    for k in _ks(n, seed):
        want_c = sigma_coeff(h, k, e.P)
        assert np.array_equal(e.to_host(e.automorphism(d, k)), want_c), ("coeff", k)
        assert np.array_equal(e.to_host(e.automorphism(d, k, ntt=True)), sigma_ntt(h, k)), ("ntt", k)


@pytest.mark.parametrize("n", [4, 1024, 4096, 16384, 32768, 65536])
@pytest.mark.parametrize("nm", [1, 4, 30])
def test_u64_degrees_and_moduli(n, nm, engine_factory):
    e = engine_factory(64, n, nm)
    for batch in (1, 3):
        d = e.fill_uniform(e.empty(batch), 11 + batch, 0)
        _check(e, d, n, batch)


@pytest.mark.parametrize("lb,n,nm", [(64, 1024, 94), (32, 1024, 2), (32, 4096, 3), (16, 128, 1), (16, 4, 2), (32, 4, 1)])
def test_other_limbs_and_moduli_past_the_92nd(lb, n, nm, engine_factory):
    e = engine_factory(lb, n, nm)
    for batch in (1, 3):
        _check(e, e.fill_uniform(e.empty(batch), 5, 1), n, 7)


def test_large_batch_u64_4096_4(engine_factory):
    import torch
    e = engine_factory(64, 4096, 4)
    d = e.fill_uniform(e.empty(16384), 3, 0)
    h = e.to_host(d)
    out = torch.empty_like(d)
    for k in (5, 8191):
        e.automorphism(d, k, out=out)
        assert np.array_equal(e.to_host(out), sigma_coeff(h, k, e.P))
        e.automorphism(d, k, ntt=True, out=out)
        assert np.array_equal(e.to_host(out), sigma_ntt(h, k))


def test_misaligned_operands_take_the_word_path(engine_factory):
    """pointers that are not 16-byte aligned (an offset view of a larger buffer) are served word by word"""
    import torch
    e = engine_factory(64, 1024, 2)
    words = 3 * 2 * 1024
    src = torch.zeros(words + 1, dtype=torch.int64, device="cuda:0")
    dst = torch.zeros(words + 1, dtype=torch.int64, device="cuda:0")
    a = e.fill_uniform(e.empty(3), 9, 0)
    src[1:].copy_(a.view(-1))
    h = e.to_host(a)
    for ntt in (False, True):
        e.automorphism(src[1:], 7, ntt=ntt, out=dst[1:])
        got = e.to_host(dst[1:]).reshape(h.shape)
        assert np.array_equal(got, sigma_ntt(h, 7) if ntt else sigma_coeff(h, 7, e.P))


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (64, 65536, 2), (32, 1024, 2), (16, 128, 1), (64, 1024, 94)])
def test_ntt_form_through_the_device_transforms(lb, n, nm, engine_factory):
    e = engine_factory(lb, n, nm)
    x = e.fill_uniform(e.empty(2), 4, 0)
    X = e.ntt_(x.clone())
    for k in (3, 2 * n - 1, 2 * n + 7):
        assert np.array_equal(e.to_host(e.intt_(e.automorphism(X, k, ntt=True))), e.to_host(e.automorphism(x, k)))


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (64, 16384, 2), (64, 65536, 2), (32, 1024, 2), (16, 128, 1), (64, 4, 3)])
def test_multi_form_equals_single_calls(lb, n, nm, engine_factory):
    e = engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(3), 2, 0)
    rnd = np.random.RandomState(n)
    for count in (1, 8, 16):
        ks = [int(rnd.randint(0, 2 * n)) | 1 for _ in range(count)]
        for ntt in (False, True):
            outs = e.automorphism_multi(d, ks, ntt=ntt)
            for k, o in zip(ks, outs):
                assert np.array_equal(e.to_host(o), e.to_host(e.automorphism(d, k, ntt=ntt))), (count, k, ntt)


@pytest.mark.parametrize("lb,n,nm,batch", [(64, 4096, 4, 3), (64, 4096, 4, 300), (32, 1024, 2, 5), (16, 128, 1, 2)])
def test_host_variant_equals_device_variant(lb, n, nm, batch, engine_factory):
    """batch 300 at u64/4096/4 (37.5 MiB) goes through the pipelined host path, the others through the staged one"""
    e = engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(batch), 8, 0)
    h = e.to_host(d)
    for ntt in (False, True):
        for k in (3, 2 * n - 1):
            assert np.array_equal(e.h_automorphism(h, k, ntt=ntt), e.to_host(e.automorphism(d, k, ntt=ntt)))
    # out == in is allowed on the host path (it stages)
    from nfllib_amd import _lib
    same = h.copy()
    assert _lib.lib.nflhip_automorphism(e.ctx, same.ctypes.data, same.ctypes.data, batch, 5, 0) == 0
    assert np.array_equal(same, sigma_coeff(h, 5, e.P))


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    L, ERR = _lib.lib, _lib.ERR_INVALID
    e = engine_factory(64, 1024, 2)
    d = e.fill_uniform(e.empty(4), 1, 0)
    o = torch.empty_like(d)
    p, q = d.data_ptr(), o.data_ptr()
    pb = e.bytes_per_poly
    assert L.nflhip_automorphism_dev(e.ctx, q, p, 4, 4, 0, None) == ERR                 # even k
    assert L.nflhip_automorphism_dev(e.ctx, q, p, 4, 3, 2, None) == ERR                 # unknown form
    assert L.nflhip_automorphism_dev(e.ctx, None, p, 4, 3, 0, None) == ERR              # NULL output
    assert L.nflhip_automorphism_dev(e.ctx, q, None, 4, 3, 0, None) == ERR              # NULL input
    assert L.nflhip_automorphism_dev(None, q, p, 4, 3, 0, None) == ERR                  # NULL context
    assert L.nflhip_automorphism_dev(e.ctx, p, p, 4, 3, 0, None) == ERR                 # out == in
    assert L.nflhip_automorphism_dev(e.ctx, p + pb, p, 2, 3, 1, None) == ERR            # out overlaps in
    assert L.nflhip_automorphism_dev(e.ctx, p, p + pb, 2, 3, 1, None) == ERR
    assert L.nflhip_automorphism_dev(e.ctx, p + 2 * pb, p, 2, 3, 1, None) == 0          # adjacent: no overlap
    ptrs = (C.c_void_p * 17)(*([q] + [q + pb * 0] * 16))
    ks = (C.c_uint64 * 17)(*([3] * 17))
    assert L.nflhip_automorphism_multi_dev(e.ctx, ptrs, ks, 0, p, 1, 0, None) == ERR    # count 0
    many = [torch.empty_like(d) for _ in range(17)]
    ptrs17 = (C.c_void_p * 17)(*[t.data_ptr() for t in many])
    assert L.nflhip_automorphism_multi_dev(e.ctx, ptrs17, ks, 17, p, 4, 0, None) == ERR  # above the maximum
    assert L.nflhip_automorphism_multi_dev(e.ctx, ptrs17, ks, 16, p, 4, 0, None) == 0   # the maximum itself
    two = (C.c_void_p * 2)(q, q + pb)
    assert L.nflhip_automorphism_multi_dev(e.ctx, two, ks, 2, p, 2, 0, None) == ERR     # outputs overlap
    two = (C.c_void_p * 2)(q, p)
    assert L.nflhip_automorphism_multi_dev(e.ctx, two, ks, 2, p, 2, 0, None) == ERR     # an output is the input
    bad_k = (C.c_uint64 * 2)(3, 6)
    two = (C.c_void_p * 2)(q, many[0].data_ptr())
    assert L.nflhip_automorphism_multi_dev(e.ctx, two, bad_k, 2, p, 2, 0, None) == ERR   # one even k
    assert L.nflhip_automorphism_multi_dev(e.ctx, None, ks, 1, p, 2, 0, None) == ERR     # NULL arrays
    assert L.nflhip_automorphism_multi_dev(e.ctx, two, None, 1, p, 2, 0, None) == ERR
    null_out = (C.c_void_p * 1)(None)
    assert L.nflhip_automorphism_multi_dev(e.ctx, null_out, ks, 1, p, 2, 0, None) == ERR
    h = e.to_host(d)
    hp = h.ctypes.data
    ho = np.empty_like(h)
    assert L.nflhip_automorphism(e.ctx, ho.ctypes.data, hp, 4, 2, 0) == ERR               # host: even k
    assert L.nflhip_automorphism(e.ctx, ho.ctypes.data, hp, 4, 3, 5) == ERR               # host: unknown form
    assert L.nflhip_automorphism(e.ctx, None, hp, 4, 3, 0) == ERR                         # host: NULL
    assert L.nflhip_automorphism(e.ctx, hp + pb, hp, 2, 3, 0) == ERR                      # host: partial overlap
    # nothing above wrote anything it should not have, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(d), h)
    assert np.array_equal(e.to_host(e.automorphism(d, 3)), sigma_coeff(h, 3, e.P))


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (64, 65536, 2), (32, 1024, 2)])
def test_graph_capture_replays_identically(lb, n, nm, engine_factory):
    import torch
    e = engine_factory(lb, n, nm)
    a = e.fill_uniform(e.empty(4), 6, 0)
    h = e.to_host(a)
    x, y = e.empty(4), e.empty(4)
    outs = [e.empty(4) for _ in range(3)]
    ks = [3, 5, 2 * n - 1]
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        e.automorphism(a, 7, out=x)
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            e.automorphism(a, 7, out=x)
            e.automorphism(x, 3, ntt=True, out=y)
            e.automorphism_multi(a, ks, outs=outs)
    for _ in range(3):
        for t in [x, y] + outs:
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(x), sigma_coeff(h, 7, e.P))
        assert np.array_equal(e.to_host(y), sigma_ntt(sigma_coeff(h, 7, e.P), 3))
        for k, o in zip(ks, outs):
            assert np.array_equal(e.to_host(o), sigma_coeff(h, k, e.P))


@pytest.mark.parametrize("lb,n,nm", [(64, 4096, 4), (64, 16384, 2), (32, 1024, 2), (16, 128, 1)])
def test_ring_homomorphism_on_the_device(lb, n, nm, engine_factory, oracle_factory):
    e, o = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    a, b = e.fill_uniform(e.empty(3), 12, 0), e.fill_uniform(e.empty(3), 12, 1)
    for k in (3, 2 * n - 1):
        lhs = e.polymul(e.automorphism(a, k), e.automorphism(b, k))
        rhs = e.automorphism(e.polymul(a, b), k)
        assert np.array_equal(e.to_host(lhs), e.to_host(rhs))
        assert np.array_equal(e.to_host(rhs), sigma_coeff(o.polymul(e.to_host(a), e.to_host(b)), k, e.P))


@pytest.fixture(scope="module")
def cpp_programs(tmp_path_factory):
    from test_automorphism_cpu import build_cpp
    out = str(tmp_path_factory.mktemp("cpp_automorphism"))
    return build_cpp(out), build_cpp(out, eager=True)


@pytest.mark.parametrize("mode", ["thread0", "thread1", "eager_runtime", "eager_build"])
def test_cpp_surface_on_the_gpu(mode, cpp_programs):
    """poly, poly_p (deferred operations before and after, out == in, copy-on-write), device_batch, a one-device
    sharded_batch -- under both queue executors and with deferred execution off"""
    exe = cpp_programs[1] if mode == "eager_build" else cpp_programs[0]
    env = dict(os.environ)
    env["NFL_HIP_QUEUE_THREAD"] = "0" if mode == "thread0" else "1"
    args = [exe] + (["eager"] if mode == "eager_runtime" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
