"""GPU: the key-switch family on long rows (include/nflhip.h from "RNS base conversion and mod-down, NTT form" to "sums of ciphertext
products"; DESIGN.md 5.21 for the child contexts).  Nothing here is a new check: the restatements of tests/*_util.py and the planting and
`check` helpers of the family's own test files, at the degrees 2^13 .. 2^16 at which callers key-switch, rotate and multiply -- and at
the real row sizes of the 32- and 16-bit limbs.  Two things change with the row length:

A  which transform kernels the composed plans run on.  Above 2048 words every plan is host orchestration around nflhip_ntt_fwd_dev /
   nflhip_ntt_inv_dev on child contexts (bcn_child, kept_rows_child, level_child, the rescale children), and the child's shape picks
   the kernel: u64 8192 / 16384 row-resident, 32768 rows32k, 65536 the generic LDS + streaming passes; u32 up to 4096 generated, above
   generic; u16 128 generated, above generic.  Up to 2048 words the one-launch kernels serve: here with 32-bit words at real sizes.
B  the chunk geometry of k_permute_add_ntt, k_permute_mac_ntt and the several-output kernel: a row longer than 16 KiB is cut into 2^c
   chunks, and a k in the place of k^-1, or a chunk base that is only right for chunks 0 and 1, shows from 8 chunks on with a
   multiplier whose square is not 1 mod 16 (tests/test_automorphism_chunks_cpu.py has the premise).

Every comparison is exact equality of every word.  The helpers plant batches of 3 (edge values, the centred band, every y_i = p_i - 1,
one polynomial each), so A runs batches of 3 where it goes through them and 2 where it calls directly; B runs batch 1."""
import numpy as np
import pytest

import baseconv_util as B
import scale_round_util as S
import test_gpu_automorphism_mac as MAC
import test_gpu_baseconv_ntt as BN
import test_gpu_bsgs as BS
import test_gpu_keyswitch as KS
import test_gpu_level as LV
import test_gpu_level_rotate as LR
import test_gpu_lintrans as LT
import test_gpu_mulrelin as MR
import test_gpu_mulrelin_dot as MD
import test_gpu_rotate as RT
from bsgs_util import bsgs_level_rns, mac_multi_rns
from keyswitch_util import digits
from level_util import gather_key, level_rows
from lintrans_util import mac_rns
from mulrelin_dot_util import mulrelin_dot_rns, operand
from mulrelin_util import tensor_rns

pytestmark = pytest.mark.gpu

LDS = 65536
CHUNK = 16384                                                 # kNttChunkBytes
FAST_ROUND, CENTRED_FLOOR = (False, False), (True, True)      # (centered, floor)
SHAPES = [(64, 8192), (64, 16384), (64, 32768), (64, 65536), (32, 1024), (32, 2048), (32, 4096), (32, 8192), (16, 128), (16, 256)]
LEVEL_SHAPES = [(64, 16384), (32, 4096)]
CHUNKED = [(64, 16384, 8), (64, 65536, 32), (32, 32768, 8)]
shapes = pytest.mark.parametrize("lb,n", SHAPES, ids=lambda v: str(v))
modes = pytest.mark.parametrize("mode", [FAST_ROUND, CENTRED_FLOOR], ids=["fast-round", "centred-floor"])


def geometry(lb):
    """(nm, K, alpha): L = 3, two digits, the last one short; the 16-bit parameter set has two moduli, so L = 1 there"""
    return (4, 1, 2) if lb != 16 else (2, 1, 1)


def keyswitch_fits(lb, n, L, dnum, centered):
    """the stated bound of the one-launch key switch and multiplication (include/nflhip.h): rows of at most 2048 words and
    (L + 1) n sizeof(T) + [centred] 2 dnum n <= 64 KiB"""
    return n <= 2048 and (L + 1) * n * (lb // 8) + (2 * dnum * n if centered else 0) <= LDS


def conversion_fits(lb, n, ks, extra):
    """the stated bound of the one-launch conversion: (ks + 1 + [centred]) rows within 64 KiB"""
    return (ks + 1 + extra) * n * (lb // 8) <= LDS


def refused(call):
    from nfllib_amd import _lib
    with pytest.raises(_lib.NflHipError) as err:
        call()
    assert err.value.code == _lib.ERR_UNSUPPORTED


# ---- A: the family on every transform kernel ----
@shapes
def test_mod_up_and_mod_down(lb, n, engine_factory, oracle_factory):
    """baseconv_ntt / mod_up_ntt of the first digit, centred and fast, and mod_down_ntt by K, both roundings: the composed plan, the
    default, and the one-launch kernel where its rows fit in both modes (forced past the bound it is refused)"""
    nm, K, alpha = geometry(lb)
    e, orc, ok = engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K)
    src = (0, alpha)
    up_fits, down_fits = [conversion_fits(lb, n, alpha, c) for c in (0, 1)], [conversion_fits(lb, n, K, c) for c in (0, 1)]
    BN.check_pair(e, orc, src, (0, nm), plans=("composed", None) + (("fused",) if all(up_fits) else ()))
    a = BN.inputs(e, src)
    dA = e.to_device(orc.ntt(np.array(a)))
    for centered in (False, True):
        up = e.mod_up_ntt(dA.clone(), src, centered=centered)
        assert np.array_equal(e.to_host(up), orc.ntt(B.baseconv_rns(a, e.P, src, (0, nm), centered=centered))), centered
        if not up_fits[centered]:
            refused(lambda: e.baseconv_ntt(dA.clone(), src, (0, nm), centered=centered, plan="fused"))
    BN.check_down(e, orc, ok, K, plans=("composed", None) + (("fused",) if all(down_fits) else ()))
    dD = e.to_device(orc.ntt(np.array(BN.inputs(e, (nm - K, K), seed=6))))
    for floor in (False, True):
        if not down_fits[not floor]:
            refused(lambda: e.mod_down_ntt(dD, K, floor=floor, plan="fused"))


@modes
@shapes
def test_key_switch_every_plan_the_shape_admits(lb, n, mode, engine_factory, oracle_factory):
    """sequence, composed, the default and, within the stated LDS bound, the one-launch kernel; (fast, round) and (centred, floor).  The
    default: the one-launch kernel where it fits, else the sequence up to 2048 words and the composed plan above."""
    nm, K, alpha = geometry(lb)
    L, dnum = nm - K, len(digits(nm, K, alpha))
    e, orc, ok = engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    fits = keyswitch_fits(lb, n, L, dnum, mode[0])
    assert fits == (n <= 2048)                                       # every short row of this ladder fits, in both modes
    KS.check(e, orc, ok, K, alpha, plans=("sequence", "composed", None) + (("fused",) if fits else ()), modes=[mode])
    if not fits:
        A, Kk, _ = KS.case(e, orc, ok, K, alpha)
        refused(lambda: e.key_switch_ntt(e.to_device(A), e.to_device(Kk), K, alpha, centered=mode[0], floor=mode[1], plan="fused"))


@pytest.mark.parametrize("mode,rescale", [(FAST_ROUND, False), (CENTRED_FLOOR, True)], ids=["fast-round", "centred-floor-rescale"])
@shapes
def test_mul_relin_default_and_one_forced_plan(lb, n, mode, rescale, engine_factory, oracle_factory):
    """without the rescale in (fast, round), with it in (centred, floor); the default plan -- the one-launch kernel where it fits, else
    the merged plan -- and one forced other plan: merged where the default is the one-launch kernel, the sequence elsewhere.  L = 1
    (16-bit limbs) has no rescale: there the second case runs (centred, floor) without it."""
    nm, K, alpha = geometry(lb)
    L, dnum = nm - K, len(digits(nm, K, alpha))
    e, orc, ok, okm = MR.factories(engine_factory, oracle_factory, lb, n, nm, K)
    other = "merged" if keyswitch_fits(lb, n, L, dnum, mode[0]) else "sequence"
    MR.check(e, orc, ok, okm, K, alpha, plans=(None, other), modes=[mode], rescales=(rescale and L > 1,), squares=(False,))


@pytest.mark.parametrize("lb,n", LEVEL_SHAPES, ids=lambda v: str(v))
def test_key_switch_and_mul_relin_at_level_two(lb, n, engine_factory, oracle_factory):
    """nm = 4, K = 1, alpha = 2 at l = 2: the live rows are 0, 1 and 3, the hole is row 2, one digit.  Against the restatement on the
    gathered key, and tensor for tensor against Engine.level_engine with that key -- the definition of a level call."""
    import torch
    nm, K, alpha, level = 4, 1, 2, 2
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    assert not keyswitch_fits(lb, n, level, 1, False)
    LV.check_ks(e, orc, K, alpha, level, plans=("sequence", "composed", None), modes=[FAST_ROUND, CENTRED_FLOOR])
    ins, Kk, _, want = LV.case(e, orc, K, alpha, level)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    w = want(True, True, True, False)
    c = e.level_engine(level, K)
    try:
        assert c.P == [e.P[j] for j in level_rows(nm, K, level)]
        gK = c.to_device(gather_key(Kk, nm, K, alpha, level))
        for plan in (None, "sequence"):
            a = e.mul_relin_ntt(d[0], d[1], d[2], d[3], dK, K, alpha, rescale=True, centered=True, floor=True, plan=plan, level=level)
            b = c.mul_relin_ntt(d[0], d[1], d[2], d[3], gK, K, alpha, rescale=True, centered=True, floor=True, plan=plan)
            assert a[0].shape == a[1].shape == (3, level - 1, n)
            assert np.array_equal(e.to_host(a[0]), w[0]) and np.array_equal(e.to_host(a[1]), w[1]), plan
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), plan
        a, b = e.key_switch_ntt(d[1], dK, K, alpha, centered=True, level=level), c.key_switch_ntt(d[1], gK, K, alpha, centered=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        torch.cuda.synchronize()
    finally:
        c.close()
    for x, h in zip(d + [dK], ins + [Kk]):
        assert np.array_equal(e.to_host(x), h)


def test_bfv_tensor_at_8192(engine_factory, oracle_factory):
    """u64/8192/5, L = 2, t = 65537, batch 1, both plans of the scale-and-round: the composed scale_round_ntt plan (workspace, inverse
    transform by the context, forward transform by the child over the L rows) on the row-resident transforms"""
    n, L, nm, t = 8192, 2, 5, 65537
    e, orc, ol = engine_factory(64, n, nm), oracle_factory(64, n, nm), oracle_factory(64, n, L)
    ins = [B.random_batch(e.P[:L], n, 1, e.np_dtype, 70 + k) for k in range(4)]
    ext = []
    for x in ins:
        X = np.zeros((1, nm, n), dtype=e.np_dtype)
        X[:, :L] = ol.intt(np.array(x))
        ext.append(orc.ntt(B.baseconv_rns(X, e.P, (0, L), (0, nm), centered=True)))
    ten = tensor_rns(ext[0], ext[1], ext[2], ext[3], e.P)
    d = [e.to_device(x) for x in ins]
    for floor in (False, True):
        want = [ol.ntt(S.scale_round_rns(orc.intt(np.ascontiguousarray(c)), e.P, L, t, floor=floor)) for c in ten]
        for plan in (None, "two_pass"):
            got = e.bfv_tensor_ntt(d[0], d[1], d[2], d[3], L, t, floor=floor, plan=plan)
            assert all(g.shape == (1, L, n) and np.array_equal(e.to_host(g), w) for g, w in zip(got, want)), (floor, plan)
    for x, h in zip(d, ins):
        assert np.array_equal(e.to_host(x), h)


def test_mul_relin_dot_at_8192(engine_factory, oracle_factory):
    """u64/8192/4, K = 1, alpha = 2 at the top level: 2 groups of 3 terms, b shared by the groups; the merged sum plan, the sequence
    and the default on the row-resident transforms.  Without the rescale in (fast, round), with it in (centred, floor)."""
    n, nm, K, alpha, groups, terms = 8192, 4, 1, 2, 2, 3
    L = nm - K
    e, orc = engine_factory(64, n, nm), oracle_factory(64, n, nm)
    ins = [B.random_batch(e.P[:L], n, groups * terms if t < 2 else terms, e.np_dtype, 60 + t) for t in range(4)]
    for m in range(L):                                                           # the largest words in group 0
        ins[0][0, m] = ins[1][0, m] = ins[2][0, m] = ins[3][0, m] = e.P[m] - 1
    Kk = B.random_batch(e.P, n, 4, e.np_dtype, 70).reshape(2, 2, nm, n)
    ops = [operand(x, groups, terms, shared=t >= 2) for t, x in enumerate(ins)]
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    for (centered, floor), rescale in ((FAST_ROUND, False), (CENTRED_FLOOR, True)):
        w = mulrelin_dot_rns(*ops, Kk, e.P, K, alpha, L, centered, floor, rescale, orc)
        for plan in MD.PLANS:
            got = e.mul_relin_dot_ntt(*d, terms, dK, K, alpha, b_shared=True, rescale=rescale, centered=centered, floor=floor, plan=plan)
            assert got[0].shape == got[1].shape == (groups, L - 1 if rescale else L, n)
            assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1]), (rescale, plan)
    for x, h in zip(d + [dK], ins + [Kk]):
        assert np.array_equal(e.to_host(x), h)


# ---- B: the chunked permutation kernels at eight chunks and more ----
def multipliers(n):
    return [3, 5, 2 * n - 1, pow(5, 7, 2 * n)]


def premises(lb, n, chunks, ks):
    """what makes the case worth its time, stated so that a later edit of the shapes cannot quietly remove it"""
    assert n * (lb // 8) // CHUNK == chunks >= 8
    assert any(k * k % 16 != 1 for k in ks)


chunked = pytest.mark.parametrize("lb,n,chunks", CHUNKED, ids=lambda v: str(v))


@chunked
def test_automorphism_mac_at_eight_chunks_and_more(lb, n, chunks, engine_factory):
    """k_permute_mac_ntt, the one-buffer and the double-buffered instance: 3 terms over every window of (3, 5, 2n - 1, 5^7), the addend
    aliased to the output; nm = 4, batch 1"""
    e = engine_factory(lb, n, 4)
    ins, ws = MAC.operands(e, 4, 3, 1)
    add = B.random_batch(e.P, n, 1, e.np_dtype, 999)
    di, dw = [e.to_device(x) for x in ins], [e.to_device(w) for w in ws]
    for ks in (multipliers(n)[:3], multipliers(n)[1:]):
        premises(lb, n, chunks, ks)
        want = mac_rns(ins, ws, ks, e.P, addend=add)
        for double in (False, True):
            out = e.to_device(add)
            got = e.automorphism_mac(di, dw, ks, addend=out, out=out, double_buffer=double)
            assert np.array_equal(e.to_host(got), want), (ks, double)
    assert all(np.array_equal(e.to_host(x), h) for x, h in zip(di + dw, ins + ws))


@chunked
def test_automorphism_mac_multi_at_eight_chunks_and_more(lb, n, chunks, engine_factory):
    """the several-output kernel: two outputs of four terms k = 3, 5, 2n - 1, 5^7, one weight None, one addend in place; nm = 4, batch 1"""
    e = engine_factory(lb, n, 4)
    ks = multipliers(n)
    premises(lb, n, chunks, ks)
    ins, _ = MAC.operands(e, 4, 4, 1, seed=5)
    ws = [[B.random_batch(e.P, n, 1, e.np_dtype, 300 + 4 * o + t)[0] for t in range(4)] for o in range(2)]
    ws[1][0] = None
    add = B.random_batch(e.P, n, 1, e.np_dtype, 77)
    want = mac_multi_rns(ins, ws, ks, e.P, addends=[None, add])
    di, dw = [e.to_device(x) for x in ins], [[None if w is None else e.to_device(w) for w in row] for row in ws]
    outs = [e.to_device(np.zeros_like(add)), e.to_device(add)]
    got = e.automorphism_mac_multi(di, dw, ks, addends=[None, outs[1]], outs=outs)
    assert all(np.array_equal(e.to_host(g), w) for g, w in zip(got, want))
    assert all(np.array_equal(e.to_host(x), h) for x, h in zip(di, ins))
    assert all(np.array_equal(e.to_host(x), h) for dr, hr in zip(dw, ws) for x, h in zip(dr, hr) if h is not None)


@chunked
def test_hoisted_rotations_at_eight_chunks_and_more(lb, n, chunks, engine_factory, oracle_factory):
    """k_permute_add_ntt, which finds its output chunk through k^-1: 4 rotations by 3, 5, 2n - 1, 5^7 with two keys, both plans and the
    default (4 rotations: hoisted); nm = 4, K = 1, alpha = 2, batch 1"""
    e, orc, ok = engine_factory(lb, n, 4), oracle_factory(lb, n, 4), oracle_factory(lb, n, 3)
    ks, which = multipliers(n), [0, 1, 0, 1]
    premises(lb, n, chunks, ks)
    c0, c1, keys, want = RT.case(e, orc, ok, 1, 2, polys=1)
    dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
    w = want(True, False, ks, which)
    for plan in RT.PLANS:
        assert RT.same(e, RT.run(e, dc0, dc1, dkeys, ks, which, 1, 2, centered=True, plan=plan), w), plan
    assert all(np.array_equal(e.to_host(x), h) for x, h in zip([dc0, dc1] + dkeys, [c0, c1] + keys))


@chunked
def test_linear_transform_at_eight_chunks_and_more(lb, n, chunks, engine_factory, oracle_factory):
    """k_permute_mac_ntt under the linear transform at the top level: 4 terms, the third unkeyed, (3, 5, 1, 2n - 1) and (5^7, 3, 1, 5);
    both plans and the default (hoisted); nm = 4, K = 1, alpha = 2, batch 1"""
    e, orc, ok = engine_factory(lb, n, 4), oracle_factory(lb, n, 4), oracle_factory(lb, n, 3)
    m = multipliers(n)
    which = [0, 1, None, 0]
    c0, c1, keys, ws, want = LT.setup(e, orc, ok, 1, 2, polys=1)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:4]]
    for ks in ([m[0], m[1], 1, m[2]], [m[3], m[0], 1, m[1]]):
        premises(lb, n, chunks, ks)
        w = want(True, False, ks, which)
        for plan in LT.PLANS:
            assert LT.same(e, LT.run(e, dc0, dc1, dkeys, dws, ks, which, 1, 2, centered=True, plan=plan), w), (ks, plan)
    assert all(np.array_equal(e.to_host(x), h) for x, h in zip([dc0, dc1] + dkeys + dws, [c0, c1] + keys + ws[:4]))


@chunked
def test_linear_transform_at_level_two_at_eight_chunks_and_more(lb, n, chunks, engine_factory, oracle_factory):
    """the level instance of k_permute_mac_ntt at l = 2 of L = 3: the per-row weight select of the chunked tiles with the hole in play.
    4 terms (3, 5, 1, 5^7), the third unkeyed; both plans and the default; nm = 4, K = 1, alpha = 2, batch 1"""
    e, orc = engine_factory(lb, n, 4), oracle_factory(lb, n, 4)
    m = multipliers(n)
    ks, which = [m[0], m[1], 1, m[3]], [0, 1, None, 0]
    premises(lb, n, chunks, ks)
    c0, c1, keys, ws, _, want = LR.case(e, orc, 1, 2, 2, polys=1)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:4]]
    w = want(True, False, ks, which)
    for plan in LT.PLANS:
        assert LR.same_lt(e, LR.run_lt(e, dc0, dc1, dkeys, dws, ks, which, 1, 2, 2, centered=True, plan=plan), w), plan
    assert all(np.array_equal(e.to_host(x), h) for x, h in zip([dc0, dc1] + dkeys + dws, [c0, c1] + keys + ws[:4]))


def test_bsgs_at_eight_chunks(engine_factory, oracle_factory):
    """u64/16384/4, K = 1, alpha = 2, batch 1, (n1, n2) = (2, 2) with the second baby step unkeyed: baby k = 3, giants 5 and
    (2n - 1) 5^7; both plans at the top level (fast, round) and at l = 2 centred, where the several-output kernel selects its weights
    per row across the hole"""
    lb, n, chunks = CHUNKED[0]
    e, orc = engine_factory(lb, n, 4), oracle_factory(lb, n, 4)
    bks, gks = [3, 1], [5, (2 * n - 1) * pow(5, 7, 2 * n) % (2 * n)]
    premises(lb, n, chunks, bks + gks)
    assert gks[1] ** 2 % 16 != 1
    for level, (centered, floor) in ((3, FAST_ROUND), (2, (True, False))):
        c0, c1, keys, ws, _ = BS.case(e, orc, 1, 2, level, polys=1)
        bkeys, gkeys = [keys[0], None], [keys[1], keys[2]]
        weights = [[ws[2 * j + i] for i in range(2)] for j in range(2)]
        dkeys, dws = [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:4]]
        dc0, dc1 = e.to_device(c0), e.to_device(c1)
        w = bsgs_level_rns(c0, c1, bkeys, bks, gkeys, gks, weights, e.P, 1, 2, level, centered, floor, orc)
        for plan in BS.PLANS + (None,):
            got = e.bsgs_linear_transform_ntt(dc0, dc1, [dkeys[0], None], bks, [dkeys[1], dkeys[2]], gks,
                                              [[dws[2 * j + i] for i in range(2)] for j in range(2)], 1, 2, centered=centered, floor=floor,
                                              plan=plan, level=level)
            assert BS.same(e, got, w), (level, plan)
        assert all(np.array_equal(e.to_host(x), h) for x, h in zip([dc0, dc1] + dkeys + dws, [c0, c1] + keys + ws[:4]))
