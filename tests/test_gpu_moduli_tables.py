"""-m gpu: every entry point at the TOP of each modulus table, against the CPU oracle word for word.

The primes are p = 2^(w-2) - delta with delta growing along each table (nfllib_amd/data/params.json): u64 #91 (the last
delta-form modulus) has delta ~ 2^32, u32 #290 has p ~ 0.81 * 2^30.  The range arguments of the 62-bit and 30-bit kernels
 have their smallest margins there.  The contexts are prefixes of the tables, as the reference declares
them (poly<uint64_t, n, 92>, poly<uint32_t, n, 291>, poly<uint64_t, n, 1000>), and the edge rows sit on the LAST moduli:
all p-1, alternating 0 / p-1, X^(n-1) * X = -1, and 0, 1, p-1 at positions 0, 1 and n-1 of every row.

Each test shows which kernels it reached: nflhip_has_fused_kernels (the generated family serves a 92-modulus u64 context,
unlike the 93+ contexts of test_gpu_big_delta.py), the one-launch counter at 32768 / 65536, and the product level switch
(complete and incomplete transforms, two kernels that must give the same words)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SEED

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
ADD, SUB, MUL = 0, 1, 2
EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_MSH, EXPR_CSH = 0x10, 0x11, 0x12, 0x13, 0x14
THREADS = 16


@pytest.fixture()
def level():
    from nfllib_amd import _lib
    saved = _lib.lib.nflhip_debug_polymul_level(-1)
    yield lambda v: _lib.lib.nflhip_debug_polymul_level(v)
    _lib.lib.nflhip_debug_polymul_level(saved)


def _fused(e):
    e.lib.nflhip_has_fused_kernels.restype = C.c_int
    return bool(e.lib.nflhip_has_fused_kernels(e.ctx))


def _launches(e):
    e.lib.nflhip_debug_xcd_launches.restype = C.c_ulonglong
    return int(e.lib.nflhip_debug_xcd_launches())


_PINNED = {}


def _pinned(n, m, xcd):
    """a u64 context whose long-row plan is pinned at creation (NFLHIP_XCD=1: the one-launch plan, 0: the others)"""
    from nfllib_amd import Engine
    key = (n, m, xcd)
    if key not in _PINNED:
        saved = os.environ.get("NFLHIP_XCD")
        os.environ["NFLHIP_XCD"] = "1" if xcd else "0"
        try:
            _PINNED[key] = Engine(64, n, m)
        finally:
            if saved is None:
                os.environ.pop("NFLHIP_XCD", None)
            else:
                os.environ["NFLHIP_XCD"] = saved
    return _PINNED[key]


@pytest.fixture(scope="module", autouse=True)
def _close_pinned():
    yield
    for e in _PINNED.values():
        e.close()
    _PINNED.clear()


def _pm1(o, dtype):
    return (np.array(o.P, dtype=np.uint64) - 1).astype(dtype)


def _inputs(o, n, batch):
    """the seeded uniform stream with the edge rows on the last moduli of the context"""
    a, b = o.fill_uniform(batch, SEED, 0), o.fill_uniform(batch, SEED, 1)
    pm1 = _pm1(o, a.dtype)
    m = len(pm1)
    a[0, :, 0], a[0, :, 1], a[0, :, n - 1] = 0, 1, pm1
    b[0, :, 0], b[0, :, 1], b[0, :, n - 1] = pm1, 0, 1
    a[0, m - 1], b[0, m - 1] = pm1[m - 1], pm1[m - 1]                                  # all p-1
    alt = np.arange(n) % 2 == 0
    a[0, m - 2] = np.where(alt, 0, pm1[m - 2])                                          # alternating 0 / p-1
    b[0, m - 2] = np.where(alt, pm1[m - 2], 0)
    a[0, m - 3], b[0, m - 3] = 0, 0                                                     # X^(n-1) * X = -1
    a[0, m - 3, n - 1], b[0, m - 3, 1] = 1, 1
    if batch > 1:
        a[batch - 1, m - 1], b[batch - 1, m - 1] = np.where(alt, pm1[m - 1], 0), pm1[m - 1]
    return a, b


def _check_products(e, o, a, b, want, level, levels=(0, 2)):
    for lv in levels:
        level(lv)
        da, db = e.to_device(a), e.to_device(b)
        assert np.array_equal(e.to_host(e.polymul(da, db)), want), "level %d" % lv
        e.polymul(da, db, out=da)
        assert np.array_equal(e.to_host(da), want), "level %d, result over a" % lv
        da = e.to_device(a)
        e.polymul(da, db, out=db)
        assert np.array_equal(e.to_host(db), want), "level %d, result over b" % lv


def _check_transforms(e, o, a, b, want):
    da, db = e.to_device(a), e.to_device(b)
    fa = e.ntt_(da.clone())
    assert np.array_equal(e.to_host(fa), o.ntt(a)), "forward"
    assert np.array_equal(e.to_host(e.intt_(da.clone())), o.intt(a)), "inverse"
    assert np.array_equal(e.to_host(e.intt_(fa.clone())), a), "round trip"
    assert np.array_equal(e.to_host(e.polymul(db, fa, b_is_ntt=True)), want), "b_is_ntt"


def _check_twin(ce, a, b, want):
    assert np.array_equal(ce.to_host(ce.polymul(ce.to_device(a), ce.to_device(b))), want), "hipcc twin"


# ------------------------------------------------------------------ u64, 92 moduli: every delta-form prime
@pytest.mark.parametrize("n", [1024, 2048, 8192, 16384, 32768, 65536])
def test_u64_every_delta_form_modulus(n, level, oracle_factory, engine_factory, compiled_engine_factory):
    import torch
    m, batch = 92, 2
    o = oracle_factory(64, n, m)
    assert (1 << 62) - o.P[m - 1] < (1 << 32), "#91 is no longer a delta-form modulus"
    a, b = _inputs(o, n, batch)
    want = o.polymul_mt(a, b, THREADS)
    if n <= 32768:
        e = engine_factory(64, n, m)
        assert _fused(e), "a 92-modulus context must be served by the generated kernels"
        _check_products(e, o, a, b, want, level)
        _check_transforms(e, o, a, b, want)
    if n >= 32768:                       # both long-row plans, pinned, and the counter shows which one ran
        for xcd in (False, True):
            e = _pinned(n, m, xcd)
            for lv in (0, 2):
                level(lv)
                before = _launches(e)
                got = e.polymul(e.to_device(a), e.to_device(b))
                torch.cuda.synchronize()
                assert (_launches(e) - before == 1) == xcd, "the plan under test did not run"
                assert np.array_equal(e.to_host(got), want), (xcd, lv)
            if n == 65536 and not xcd:
                _check_transforms(e, o, a, b, want)
    _check_twin(compiled_engine_factory(64, n, m), a, b, want)


def _fused_entries(e, o, n, batch, fmt, ce=None):
    """fwd_fma / fwd_fma2 (word and int8 operands; shared and dense keys) and fma_inv (subtract / add) against the oracle run
    operator by operator, as tests/test_gpu_fused.py does at fewer moduli"""
    import torch
    P = np.array(o.P, dtype=np.uint64)
    pm1 = _pm1(o, e.np_dtype)
    ka, kb = o.fill_uniform(1, 7, 0), o.fill_uniform(1, 7, 1)
    ka[0, -1], kb[0, -2, ::2] = pm1[-1], pm1[-2]
    if fmt == "words":
        w = [o.fill_uniform(batch, 11 + i, i & 1) for i in range(3)]
        w[0][0, -1] = pm1[-1]
        w[1][0, -2] = np.where(np.arange(n) % 2 == 0, pm1[-2], 0)
        xs = [e.to_device(x) for x in w]
    else:
        rng = np.random.default_rng(n + len(P))
        small = [rng.integers(-128, 127, size=(batch, n), endpoint=True).astype(np.int8) for _ in range(3)]
        small[0][0, :4] = (-128, 127, 0, -1)
        w = [np.where(x.astype(np.int64)[:, None, :] < 0, P[None, :, None].astype(np.int64) + x.astype(np.int64)[:, None, :],
                      x.astype(np.int64)[:, None, :]).astype(e.np_dtype) for x in small]
        xs = [torch.from_numpy(x).to("cuda:0") for x in small]
    bc = lambda k: np.ascontiguousarray(np.broadcast_to(k, w[0].shape))
    f = [o.ntt(x) for x in w]
    want0 = o.pointwise(ADD, o.pointwise(MUL, f[0], bc(ka)), f[1])
    want1 = o.pointwise(ADD, o.pointwise(MUL, f[0], bc(kb)), f[2])
    dka, dkb = e.to_device(ka), e.to_device(kb)
    got0, got1 = e.fwd_fma2(xs[0], dka, xs[1], dkb, xs[2])
    assert np.array_equal(e.to_host(got0), want0) and np.array_equal(e.to_host(got1), want1), "fwd_fma2"
    assert np.array_equal(e.to_host(e.fwd_fma(xs[0], dkb, xs[2])), want1), "fwd_fma, shared key"
    dense = o.fill_uniform(batch, 19, 1)
    dense[-1, -1] = pm1[-1]
    want = o.pointwise(ADD, o.pointwise(MUL, f[0], dense), f[1])
    assert np.array_equal(e.to_host(e.fwd_fma(xs[0], e.to_device(dense), xs[1])), want), "fwd_fma, a key per element"
    if ce is not None:
        c0, c1 = ce.fwd_fma2(xs[0], dka, xs[1], dkb, xs[2])
        assert torch.equal(c0, got0) and torch.equal(c1, got1), "hipcc twin"
    if fmt == "words":
        prod = o.pointwise(MUL, w[0], bc(ka))
        for sub in (True, False):
            want = o.intt(o.pointwise(SUB if sub else ADD, w[1], prod))
            assert np.array_equal(e.to_host(e.fma_inv(xs[0], dka, xs[1], subtract=sub)), want), ("fma_inv", sub)
        prod = o.pointwise(MUL, w[0], dense)
        want = o.intt(o.pointwise(SUB, w[1], prod))
        assert np.array_equal(e.to_host(e.fma_inv(xs[0], e.to_device(dense), xs[1], subtract=True)), want), "fma_inv, dense key"


@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192, 16384, 32768])
@pytest.mark.parametrize("fmt", ["words", "i8"])
def test_u64_fused_entries_on_every_delta_form_modulus(n, fmt, oracle_factory, engine_factory):
    m = 92
    e, o = engine_factory(64, n, m), oracle_factory(64, n, m)
    assert _fused(e), "the generated fused kernels must serve this context"
    _fused_entries(e, o, n, 2, fmt)


# ------------------------------------------------------------------ u32, 291 moduli: the whole table
@pytest.mark.parametrize("n", [8, 1024, 2048, 4096, 8192, 32768])
def test_u32_whole_table(n, level, oracle_factory, engine_factory, compiled_engine_factory):
    m, batch = 291, 2
    o, e = oracle_factory(32, n, m), engine_factory(32, n, m)
    assert _fused(e) == (1024 <= n <= 4096), "the wave-per-row kernels serve exactly the rows of 1024 .. 4096 words"
    a, b = _inputs(o, n, batch)
    want = o.polymul_mt(a, b, THREADS)
    _check_products(e, o, a, b, want, level)
    _check_transforms(e, o, a, b, want)
    _check_twin(compiled_engine_factory(32, n, m), a, b, want)


@pytest.mark.parametrize("n", [1024, 2048, 4096])
@pytest.mark.parametrize("fmt", ["words", "i8"])
def test_u32_fused_entries_on_the_whole_table(n, fmt, oracle_factory, engine_factory, compiled_engine_factory):
    m = 291
    e, o = engine_factory(32, n, m), oracle_factory(32, n, m)
    assert _fused(e)
    _fused_entries(e, o, n, 2, fmt, ce=compiled_engine_factory(32, n, m))


# ------------------------------------------------------------------ u64, 1000 moduli: past the delta form
@pytest.mark.parametrize("n", [8, 1024, 4096])
def test_u64_whole_table(n, oracle_factory, engine_factory):
    """at 4096 the per-row split: rows 0..91 on the delta-form kernels, 92..999 on the general ones"""
    m, batch = 1000, 1
    o, e = oracle_factory(64, n, m), engine_factory(64, n, m)
    a, b = _inputs(o, n, batch)
    want = o.polymul_mt(a, b, THREADS)
    da, db = e.to_device(a), e.to_device(b)
    assert np.array_equal(e.to_host(e.polymul(da, db)), want)
    fa = e.ntt_(da.clone())
    assert np.array_equal(e.to_host(fa), o.ntt(a))
    assert np.array_equal(e.to_host(e.intt_(da.clone())), o.intt(a))
    assert np.array_equal(e.to_host(e.intt_(fa)), a)


# ------------------------------------------------------------------ the modulus-indexed entries on short rows
@pytest.mark.parametrize("lb,m", [(32, 291), (64, 1000)])
def test_modulus_indexed_entries_on_the_whole_table(lb, m, oracle_factory, engine_factory):
    from nfllib_amd import DIST_BOUNDED, DIST_UNIFORM, DIST_ZO, OP_ADD, OP_COMPUTE_SHOUP, OP_MUL, OP_MUL_SHOUP, OP_SUB
    from oracle import samplers as S
    n, batch = 64, 2
    o, e = oracle_factory(lb, n, m), engine_factory(lb, n, m)
    P = [int(p) for p in o.P]
    a, b = _inputs(o, n, batch)
    c = o.fill_uniform(batch, 77, 0)
    da, db, dc = e.to_device(a), e.to_device(b), e.to_device(c)
    # point-wise operators and expression trees
    for op in (OP_ADD, OP_SUB, OP_MUL):
        assert np.array_equal(e.to_host(e.pointwise(op, da, db)), o.pointwise(op, a, b)), op
    bp = o.pointwise(OP_COMPUTE_SHOUP, b)
    dbp = e.pointwise(OP_COMPUTE_SHOUP, db)
    assert np.array_equal(e.to_host(dbp), bp)
    assert np.array_equal(e.to_host(e.pointwise(OP_MUL_SHOUP, da, db, dbp)), o.pointwise(OP_MUL_SHOUP, a, b, bp))
    want = o.pointwise(OP_SUB, b, o.pointwise(OP_MUL, a, c))
    assert np.array_equal(e.to_host(e.eval([1, 0, 2, EXPR_MUL, EXPR_SUB], [da, db, dc])), want)
    want = o.pointwise(OP_ADD, o.pointwise(OP_MUL, a, b), c)
    assert np.array_equal(e.to_host(e.eval([0, 1, 1, EXPR_CSH, EXPR_MSH, 2, EXPR_ADD], [da, db, dc])), want)
    # the seeded uniform stream
    assert np.array_equal(e.to_host(e.fill_uniform(e.empty(batch), SEED, 1)), o.fill_uniform(batch, SEED, 1))
    # comparisons: one equal / one different word in the LAST row
    assert e.any_neq(da, dc) and not e.any_neq(da, da) and e.any_eq(da, da)
    d2 = dc.clone()
    d2[d2 == da] += 1
    assert not e.any_eq(da, d2)
    d2[batch - 1, m - 1, n - 1] = da[batch - 1, m - 1, n - 1]
    assert e.any_eq(da, d2)
    d3 = da.clone()
    d3[batch - 1, m - 1, n - 1] ^= 1
    assert e.any_neq(da, d3)
    # the range check: canonical words pass, ONE word of the last row at p fails
    assert not e.check_range(da)
    bad = a.copy()
    bad[batch - 1, m - 1, n // 2] = P[m - 1]
    assert e.check_range(e.to_device(bad))
    bad[batch - 1, m - 1, n // 2] = P[m - 1] - 1
    assert not e.check_range(e.to_device(bad))
    # the cyclic transform of one modulus' rows (core::ntt), on the last modulus
    x = np.ascontiguousarray(a[:, m - 1, :])
    for inv in (False, True):
        want = np.stack([o.ntt_row(r, m - 1, inv) for r in x])
        assert np.array_equal(e.to_host(e.ntt_row_(e.to_device(x), m - 1, inverse_tables=inv)), want), inv
    # samplers against the reference's rules fed with the very keystream words
    dt = e.np_dtype
    mask = (1 << lb) - 1
    words = (S.chacha20_words(KEY, 3, 0, batch * m * n, counter_base=S.domain_base("uniform")) & np.uint64(mask)).astype(dt)
    assert np.array_equal(e.to_host(e.sample(e.empty(batch), DIST_UNIFORM, KEY, stream_id=3)), S.uniform(words.reshape(batch, m, n), P))
    lanes = S.uniform_narrow_words(KEY, 3, 0, batch * m * n, lb).reshape(batch, m, n)
    assert np.array_equal(e.to_host(e.sample(e.empty(batch), DIST_UNIFORM, KEY, stream_id=3, narrow=True)), S.uniform(lanes, P))
    cw = S.chacha20_words(KEY, 2, 0, batch * n, counter_base=S.domain_base("bounded")).reshape(batch, n)
    zw = S.chacha20_words(KEY, 2, 0, batch * n, counter_base=S.domain_base("zo")).reshape(batch, n)
    for ub, amp in ((1, 1), (5, 3), (1 << 12, 1)):
        got = e.to_host(e.sample(e.empty(batch), DIST_BOUNDED, KEY, stream_id=2, param0=ub, param1=amp))
        assert np.array_equal(got, S.non_uniform(cw, P, ub, amp, dtype=dt)), (ub, amp)
    for rho in (0x7F, 255):
        got = e.to_host(e.sample(e.empty(batch), DIST_ZO, KEY, stream_id=2, param0=rho))
        assert np.array_equal(got, S.zo_dist(zw & np.uint64(0xFF), P, rho, canonical=True, dtype=dt)), rho
