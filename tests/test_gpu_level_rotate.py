"""GPU: hoisted rotations and slot linear transforms below the top level with the ONE top-level Galois key per rotation and the ONE
top-level diagonal per term (include/nflhip.h "rotations and linear transforms at a level", nfllib_amd/csrc/kernels_level_rotate.hip).
Every plan, both mod-up modes, both roundings, word for word against tests/level_rotate_util.py: the existing restatements
rotate_rns / lintrans_rns on the moduli of the live rows A_l with the gathered keys and weights -- the header's definition of a level
call.  No tolerance anywhere.  c1 is a batch of 3 planted per LIVE digit as tests/test_gpu_level.py plants it; c0, the two keys and
the 16 diagonals are those of tests/test_gpu_rotate.py and tests/test_gpu_lintrans.py at the top level.  "Dead" are the rows [l, L) of
every key and diagonal and the digits >= dnum_l of every key, which no level-l call may read."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits
from level_rotate_util import gather_weight, lintrans_level_rns, rotate_level_rns
from level_util import RowsOracle, gather_key, level_digits
from test_gpu_keyswitch import planted
from test_gpu_level import level_view
from test_gpu_lintrans import diagonals, terms_of
from test_gpu_rotate import MODES, PICK, PLANS, rotations

pytestmark = pytest.mark.gpu

_CACHE = {}
SHAPES = [(64, 64, 6, 2, 2, 1), (64, 64, 6, 2, 2, 2), (64, 64, 6, 2, 2, 3), (64, 64, 5, 2, 1, 2), (32, 128, 4, 1, 1, 1), (32, 128, 4, 1, 1, 2),
          (64, 64, 20, 2, 1, 8), (64, 64, 20, 2, 1, 9), (64, 64, 20, 2, 1, 17)]


def case(e, orc, K, alpha, level, seed=3, polys=3):
    """c0, c1 = [polys, l, n] in NTT form (c1 planted per live digit), two TOP-LEVEL keys, the 16 top-level diagonals and, computed on
    demand and kept, the expected words"""
    ck = (e.limb_bits, e.degree, e.nmoduli, K, alpha, level, seed, polys)
    if ck not in _CACHE:
        nm, n = e.nmoduli, e.degree
        dnum = len(digits(nm, K, alpha))
        kept = RowsOracle(orc, nm, range(level))
        c1 = kept.ntt(planted(level_view(e, K, level), K, alpha, seed)[:polys])
        c0 = B.random_batch(e.P[:level], n, polys, e.np_dtype, seed + 50)
        c0[0, :, :2] = np.array([int(p) - 1 for p in e.P[:level]], dtype=e.np_dtype)[:, None]      # the sum's wrap: p - 1 + anything
        c0[-1, :, -1] = 0
        keys = [B.random_batch(e.P, n, 2 * dnum, e.np_dtype, seed + 100 + i).reshape(dnum, 2, nm, n) for i in range(2)]
        for x in [c0, c1] + keys:
            x.setflags(write=False)
        _CACHE[ck] = (c0, c1, keys, {})
    c0, c1, keys, memo = _CACHE[ck]
    ws = diagonals(e)

    def want_rot(centered, floor, ks, which, with_c0=True, pick=None):
        m = memo.setdefault(("rot", centered, floor), {})
        r = rotate_level_rns(c0 if with_c0 else None, c1, [keys[i] for i in which], ks, e.P, K, alpha, level, centered, floor, orc, memo=m)
        return r if pick is None else [(a[pick], b[pick]) for a, b in r]

    def want_lt(centered, floor, ks, which, with_c0=True, pick=None):
        m = memo.setdefault(("lt", centered), {})
        r = lintrans_level_rns(c0 if with_c0 else None, c1, [None if i is None else keys[i] for i in which], ws[:len(ks)], ks, e.P, K, alpha,
                               level, centered, floor, orc, memo=m)
        return r if pick is None else (r[0][pick], r[1][pick])
    return c0, c1, keys, ws, want_rot, want_lt


def run_rot(e, dc0, dc1, dkeys, ks, which, K, alpha, level, **kw):
    return e.rotate_hoisted_ntt(dc0, dc1, [dkeys[i] for i in which], ks, K, alpha, level=level, **kw)


def run_lt(e, dc0, dc1, dkeys, dws, ks, which, K, alpha, level, **kw):
    return e.linear_transform_ntt(dc0, dc1, [None if i is None else dkeys[i] for i in which], dws[:len(ks)], ks, K, alpha, level=level, **kw)


def same_rot(e, got, want):
    return len(got) == len(want) and all(np.array_equal(e.to_host(g[c]).reshape(w[c].shape), w[c]) for g, w in zip(got, want) for c in (0, 1))


def same_lt(e, got, want):
    return all(np.array_equal(e.to_host(got[c]).reshape(want[c].shape), want[c]) for c in (0, 1))


def check(e, orc, K, alpha, level, modes, combos, plans=PLANS, unkeyed=()):
    """both entries over (count, batch) x modes x plans; the inputs, keys and weights are unchanged afterwards"""
    c0, c1, keys, ws, want_rot, want_lt = case(e, orc, K, alpha, level)
    dkeys, dws = [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    for count, batch in combos:
        pick = PICK[batch]
        dc0, dc1 = e.to_device(c0[pick]), e.to_device(c1[pick])
        ks, which = rotations(e.degree, count)
        lks, lwhich = terms_of(e.degree, count, [m for m in unkeyed if m < count])
        for centered, floor in modes:
            wr, wl = want_rot(centered, floor, ks, which, pick=pick), want_lt(centered, floor, lks, lwhich, pick=pick)
            for plan in plans:
                got = run_rot(e, dc0, dc1, dkeys, ks, which, K, alpha, level, centered=centered, floor=floor, plan=plan)
                assert got[0][0].shape == dc1.shape == (batch, level, e.degree)
                assert same_rot(e, got, wr), ("rotate", K, alpha, level, count, batch, centered, floor, plan)
                got = run_lt(e, dc0, dc1, dkeys, dws, lks, lwhich, K, alpha, level, centered=centered, floor=floor, plan=plan)
                assert got[0].shape == got[1].shape == dc1.shape
                assert same_lt(e, got, wl), ("lintrans", K, alpha, level, count, batch, centered, floor, plan)
        assert np.array_equal(e.to_host(dc0), c0[pick]) and np.array_equal(e.to_host(dc1), c1[pick])
    assert all(np.array_equal(e.to_host(d), h) for d, h in zip(dkeys + dws, keys + ws))


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", SHAPES)
def test_every_plan_both_modes_both_roundings_every_count(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """u64/64/6 (2, 2): l = 1 has a digit shorter than alpha, l = 2 one digit fewer than the top, l = 3 a short last digit that is full
    at the top; u64/64/5 (2, 1); u32/128/4: the other limb width; u64/64/20 (2, 1): l = 8 the register form of k_dot_multi at its last
    size, l = 9 the streaming form at its first, l = 17 across the 16-term chunk of dot_reduce.h with the hole right behind the
    digits.  Rows of 512 bytes put 32 rows in a tile of k_permute_mac_ntt, so every tile here straddles the split: the per-item
    weight select.  count in {1, 2, 16}, batch 3 (G = 2 with one tile not full)."""
    check(engine_factory(lb, n, nm), oracle_factory(lb, n, nm), K, alpha, level, MODES, [(1, 3), (2, 3), (16, 3)])


@pytest.mark.parametrize("level", [1, 3])
def test_batch_one_and_five(level, engine_factory, oracle_factory):
    """u64/64/6 (2, 2): batch 1 is G = 1, batch 5 a last tile that is not full"""
    check(engine_factory(64, 64, 6), oracle_factory(64, 64, 6), 2, 2, level, [(False, False), (True, True)], [(2, 1), (16, 5), (1, 1)])


@pytest.mark.parametrize("level", [1, 2])
def test_a_row_of_two_chunks(level, engine_factory, oracle_factory):
    """u64/4096/4, K = 1, batch 1: a 32 KiB row is two chunks, the per-tile weight select of k_permute_mac_ntt; k = 2n - 1 takes a
    tile's source from the other chunk, k = 5 from its own.  The hoisted mod-up takes the inverse-transform route here."""
    e, orc = engine_factory(64, 4096, 4), oracle_factory(64, 4096, 4)
    c0, c1, keys, ws, want_rot, want_lt = case(e, orc, 1, 1, level, polys=1)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:2]]
    ks, which = [2 * 4096 - 1, 5], [0, 1]
    for centered, floor in ((False, False), (True, True)):
        wr, wl = want_rot(centered, floor, ks, which), want_lt(centered, floor, ks, which)
        for plan in PLANS:
            assert same_rot(e, run_rot(e, dc0, dc1, dkeys, ks, which, 1, 1, level, centered=centered, floor=floor, plan=plan), wr), (centered, floor, plan)
            assert same_lt(e, run_lt(e, dc0, dc1, dkeys, dws, ks, which, 1, 1, level, centered=centered, floor=floor, plan=plan), wl), (centered, floor, plan)


# ---- shared behaviour at u64/64/6 (2, 2), l = 3 ----
def _shared(engine_factory, oracle_factory, seed=3, level=3):
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    return (e,) + case(e, orc, 2, 2, level, seed=seed)


def test_linear_transform_c0_null_unkeyed_terms_and_output_placement(engine_factory, oracle_factory):
    """c0 = None; one unkeyed term among keyed ones; only unkeyed terms; out1 adjacent to out0 (one mod-down call) and apart from it"""
    import torch
    e, c0, c1, keys, ws, want_rot, want_lt = _shared(engine_factory, oracle_factory)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    for plan in PLANS:
        ks, which = terms_of(64, 4)
        assert same_lt(e, run_lt(e, None, dc1, dkeys, dws, ks, which, 2, 2, 3, centered=True, plan=plan), want_lt(True, False, ks, which, with_c0=False)), plan
        assert same_rot(e, run_rot(e, None, dc1, dkeys, ks, which, 2, 2, 3, centered=True, plan=plan), want_rot(True, False, ks, which, with_c0=False)), plan
        ks, which = terms_of(64, 4, unkeyed=[2])
        assert same_lt(e, run_lt(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, 3, plan=plan), want_lt(False, False, ks, which)), plan
        ks, which = terms_of(64, 3, unkeyed=[0, 1, 2])
        for with_c0 in (True, False):
            got = run_lt(e, dc0 if with_c0 else None, dc1, dkeys, dws, ks, which, 2, 2, 3, plan=plan)
            assert same_lt(e, got, want_lt(False, False, ks, which, with_c0=with_c0)), (plan, with_c0)
        ks, which = terms_of(64, 5, unkeyed=[1])
        w = want_lt(False, True, ks, which)
        both = torch.zeros((2,) + c1.shape, dtype=torch.int64, device="cuda:0")
        apart = torch.zeros((3,) + c1.shape, dtype=torch.int64, device="cuda:0")
        assert same_lt(e, run_lt(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, 3, floor=True, plan=plan, out=(both[0], both[1])), w), plan
        assert same_lt(e, run_lt(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, 3, floor=True, plan=plan, out=(apart[2], apart[0])), w), plan
        assert bool((apart[1] == 0).all())


def test_the_top_level_is_the_existing_entry(engine_factory, oracle_factory):
    """u64/64/6 (2, 2), l = 4 = L: tensor for tensor the output of the call without a level"""
    import torch
    e, c0, c1, keys, ws, _, _ = _shared(engine_factory, oracle_factory, level=4)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    ks, which = rotations(64, 5)
    lks, lwhich = terms_of(64, 5, unkeyed=[3])
    for plan in PLANS:
        for centered, floor in MODES:
            top = e.rotate_hoisted_ntt(dc0, dc1, [dkeys[i] for i in which], ks, 2, 2, centered=centered, floor=floor, plan=plan)
            lev = run_rot(e, dc0, dc1, dkeys, ks, which, 2, 2, 4, centered=centered, floor=floor, plan=plan)
            assert all(torch.equal(a[c], b[c]) for a, b in zip(top, lev) for c in (0, 1)), (plan, centered, floor)
            top = e.linear_transform_ntt(dc0, dc1, [None if i is None else dkeys[i] for i in lwhich], dws[:5], lks, 2, 2, centered=centered,
                                         floor=floor, plan=plan)
            lev = run_lt(e, dc0, dc1, dkeys, dws, lks, lwhich, 2, 2, 4, centered=centered, floor=floor, plan=plan)
            assert torch.equal(top[0], lev[0]) and torch.equal(top[1], lev[1]), (plan, centered, floor)


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 3), (64, 64, 6, 2, 2, 1), (32, 128, 4, 1, 1, 2), (64, 64, 20, 2, 1, 9)])
def test_the_level_call_is_the_level_engine_with_gathered_keys_and_weights(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """the definition itself, on the device: Engine.level_engine(l, K) is a context over C_l whose calls read nothing this change adds"""
    import torch
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    c0, c1, keys, ws, _, _ = case(e, orc, K, alpha, level)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    c = e.level_engine(level, K)
    try:
        gk = [c.to_device(gather_key(k, nm, K, alpha, level)) for k in keys]
        gw = [c.to_device(gather_weight(w, nm, K, level)) for w in ws]
        al = min(alpha, level)
        for count in (1, 2, 16):
            ks, which = rotations(n, count)
            lks, lwhich = terms_of(n, count, unkeyed=[1] if count > 2 else [])
            for plan in PLANS:
                for centered, floor in MODES:
                    a = run_rot(e, dc0, dc1, dkeys, ks, which, K, alpha, level, centered=centered, floor=floor, plan=plan)
                    b = c.rotate_hoisted_ntt(dc0, dc1, [gk[i] for i in which], ks, K, al, centered=centered, floor=floor, plan=plan)
                    assert all(torch.equal(x[j], y[j]) for x, y in zip(a, b) for j in (0, 1)), (count, plan, centered, floor)
                    a = run_lt(e, dc0, dc1, dkeys, dws, lks, lwhich, K, alpha, level, centered=centered, floor=floor, plan=plan)
                    b = c.linear_transform_ntt(dc0, dc1, [None if i is None else gk[i] for i in lwhich], gw[:count], lks, K, al, centered=centered,
                                               floor=floor, plan=plan)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (count, plan, centered, floor)
        torch.cuda.synchronize()
    finally:
        c.close()


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 1), (64, 64, 6, 2, 2, 3), (32, 128, 4, 1, 1, 1)])
def test_dead_rows_and_digits_are_never_read(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """rows [l, L) of every key and weight and the digits >= dnum_l of every key hold all-ones words (no canonical residues), then
    zeros: every plan returns the restatement's words, which never saw them.  A key cut after its last live digit is accepted, and
    it lies inside a larger tensor with all-ones guard words behind it: a read of a later digit shows as wrong words."""
    import torch
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    c0, c1, keys, ws, want_rot, want_lt = case(e, orc, K, alpha, level)
    L, dl, ones = nm - K, level_digits(level, alpha), int(np.iinfo(e.np_dtype).max)
    dc0, dc1 = e.to_device(c0), e.to_device(c1)
    ks, which = rotations(n, 4)
    lks, lwhich = terms_of(n, 4, unkeyed=[2])
    wr, wl = want_rot(True, False, ks, which), want_lt(True, False, lks, lwhich)
    for value in (ones, 0):
        full, cut, dws = [], [], []
        for k in keys:
            k = np.array(k)
            k[:, :, level:L] = value
            k[dl:] = value
            full.append(e.to_device(k))
            guarded = np.full(k[:dl].size + 2 * n, ones, dtype=e.np_dtype)
            guarded[:k[:dl].size] = k[:dl].ravel()
            cut.append(e.to_device(guarded)[:k[:dl].size].view(dl, 2, nm, n))
        for w in ws[:4]:
            w = np.array(w)
            w[level:L] = value
            dws.append(e.to_device(w))
        for dkeys in (full, cut):
            for plan in PLANS:
                assert same_rot(e, run_rot(e, dc0, dc1, dkeys, ks, which, K, alpha, level, centered=True, plan=plan), wr), (plan, value)
                assert same_lt(e, run_lt(e, dc0, dc1, dkeys, dws, lks, lwhich, K, alpha, level, centered=True, plan=plan), wl), (plan, value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_c0", [True, False])
def test_every_buffer_one_word_off_alignment_with_guard_words(with_c0, engine_factory, oracle_factory):
    """the word variants of both kernels, with the hole; the inputs, keys and weights are unchanged afterwards"""
    import torch
    e, c0, c1, keys, ws, want_rot, want_lt = _shared(engine_factory, oracle_factory)
    ks, which = rotations(64, 3)
    lks, lwhich = terms_of(64, 3, unkeyed=[1])
    wr, wl = want_rot(True, False, ks, which, with_c0=with_c0), want_lt(True, False, lks, lwhich, with_c0=with_c0)

    def off(h, fill=0):
        t = torch.full((h.size + 2,), fill, dtype=torch.int64, device="cuda:0")
        t[1:-1].copy_(e.to_device(h).view(-1))
        return t
    a0, a1, ak, aw = off(c0), off(c1), [off(k) for k in keys], [off(w) for w in ws[:3]]
    d0 = a0[1:-1].view(c0.shape) if with_c0 else None
    for plan in PLANS:
        outs = [tuple(torch.full((c1.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2)) for _ in ks]
        e.rotate_hoisted_ntt(d0, a1[1:-1].view(c1.shape), [ak[i][1:-1] for i in which], ks, 2, 2, centered=True,
                             outs=[(o[0][1:-1], o[1][1:-1]) for o in outs], plan=plan, level=3)
        for o, x in zip(outs, wr):
            for c in (0, 1):
                assert np.array_equal(e.to_host(o[c][1:-1]).reshape(x[c].shape), x[c]) and int(o[c][0]) == 7 and int(o[c][-1]) == 7, plan
        o = tuple(torch.full((c1.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2))
        e.linear_transform_ntt(d0, a1[1:-1].view(c1.shape), [None if i is None else ak[i][1:-1] for i in lwhich], [w[1:-1] for w in aw], lks, 2, 2,
                               centered=True, out=(o[0][1:-1], o[1][1:-1]), plan=plan, level=3)
        for c in (0, 1):
            assert np.array_equal(e.to_host(o[c][1:-1]).reshape(wl[c].shape), wl[c]) and int(o[c][0]) == 7 and int(o[c][-1]) == 7, plan
    for t, h in [(a0, c0), (a1, c1)] + list(zip(ak, keys)) + list(zip(aw, ws[:3])):
        assert int(t[0]) == 0 and int(t[-1]) == 0 and np.array_equal(e.to_host(t[1:-1]).reshape(h.shape), h)


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, c0, c1, keys, ws, want_rot, want_lt = _shared(engine_factory, oracle_factory)
    ks, which = rotations(64, 4)
    lks, lwhich = terms_of(64, 4, unkeyed=[2])
    dl = level_digits(3, 2)
    for plan in PLANS:
        for hkeys in (keys, [np.ascontiguousarray(k[:dl]) for k in keys]):                     # the whole key, and cut after its last live digit
            h = e.h_rotate_hoisted_ntt(np.array(c0), np.array(c1), [np.array(hkeys[i]) for i in which], ks, 2, 2, centered=True, plan=plan, level=3)
            w = want_rot(True, False, ks, which)
            assert all(np.array_equal(a[c], b[c]) for a, b in zip(h, w) for c in (0, 1)), plan
            h = e.h_linear_transform_ntt(np.array(c0), np.array(c1), [None if i is None else np.array(hkeys[i]) for i in lwhich],
                                         [np.array(x) for x in ws[:4]], lks, 2, 2, centered=True, plan=plan, level=3)
            w = want_lt(True, False, lks, lwhich)
            assert np.array_equal(h[0], w[0]) and np.array_equal(h[1], w[1]), plan
        d = run_rot(e, e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], ks, which, 2, 2, 3, centered=True, plan=plan)
        assert same_rot(e, d, want_rot(True, False, ks, which))


@pytest.mark.parametrize("plan", ["sequence", "hoisted"])
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, c0, c1, keys, ws, want_rot, want_lt = _shared(engine_factory, oracle_factory)
    _, b0, b1, keys2, _, want_rot2, want_lt2 = _shared(engine_factory, oracle_factory, seed=11)
    ks, which = rotations(64, 3)
    d = [e.to_device(x) for x in (c0, c1, b0, b1)]
    dk, dk2, dws = [e.to_device(k) for k in keys], [e.to_device(k) for k in keys2], [e.to_device(w) for w in ws[:3]]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = run_rot(e, d[0], d[1], dk, ks, which, 2, 2, 3, centered=True, plan=plan, stream=s1)
        r2 = run_rot(e, d[2], d[3], dk2, ks, which, 2, 2, 3, centered=True, plan=plan, stream=s2)
        l1 = run_lt(e, d[0], d[1], dk, dws, ks, which, 2, 2, 3, centered=True, plan=plan, stream=s1)
        l2 = run_lt(e, d[2], d[3], dk2, dws, ks, which, 2, 2, 3, centered=True, plan=plan, stream=s2)
    torch.cuda.synchronize()
    assert same_rot(e, r1, want_rot(True, False, ks, which)) and same_rot(e, r2, want_rot2(True, False, ks, which))
    assert same_lt(e, l1, want_lt(True, False, ks, which)) and same_lt(e, l2, want_lt2(True, False, ks, which))


@pytest.mark.parametrize("plan", ["sequence", "hoisted"])
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, c0, c1, keys, ws, want_rot, want_lt = _shared(engine_factory, oracle_factory)
    ks, which = rotations(64, 3)
    lks, lwhich = terms_of(64, 3, unkeyed=[1])
    wr, wl = want_rot(True, False, ks, which), want_lt(True, False, lks, lwhich)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:3]]
    rot = torch.zeros((3, 2) + c1.shape, dtype=torch.int64, device="cuda:0")
    lt = torch.zeros((2,) + c1.shape, dtype=torch.int64, device="cuda:0")
    outs = [(rot[m, 0], rot[m, 1]) for m in range(3)]

    def go():
        run_rot(e, dc0, dc1, dkeys, ks, which, 2, 2, 3, centered=True, plan=plan, outs=outs)
        run_lt(e, dc0, dc1, dkeys, dws, lks, lwhich, 2, 2, 3, centered=True, plan=plan, out=(lt[0], lt[1]))

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        go()                                                   # the warm-up: the level context, its tables and scratch
        st.synchronize()
        assert same_rot(e, outs, wr) and same_lt(e, lt, wl)
        with torch.cuda.graph(g, stream=st):
            go()
    for _ in range(3):
        rot.zero_(), lt.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same_rot(e, outs, wr) and same_lt(e, lt, wl)


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e, orc = Engine(64, 64, 6, device=0), oracle_factory(64, 64, 6)   # a context of its own: no level context exists, nothing is warm
    try:
        c0, c1, keys, ws, want_rot, want_lt = case(e, orc, 2, 2, 3)
        ks, which = rotations(64, 2)
        wr, wl = want_rot(False, False, ks, which), want_lt(False, False, ks, which)
        dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:2]]
        pk = (C.c_void_p * 2)(*[dkeys[i].data_ptr() for i in which])
        pw = (C.c_void_p * 2)(*[w.data_ptr() for w in dws])
        kv = (C.c_uint64 * 2)(*ks)
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        for level, flags in ((3, _lib.ROTATE_HOISTED), (3, _lib.ROTATE_SEQUENCE), (2, 0)):   # (the level context, then each plan, is cold in its turn)
            o = torch.full((2, 2, 3, level, 64), 5, dtype=torch.int64, device="cuda:0")
            p0 = (C.c_void_p * 2)(o[0, 0].data_ptr(), o[1, 0].data_ptr())
            p1 = (C.c_void_p * 2)(o[0, 1].data_ptr(), o[1, 1].data_ptr())
            a0, a1 = (dc0, dc1) if level == 3 else (dc0[:, :2].contiguous(), dc1[:, :2].contiguous())

            def rot():
                return _lib.lib.nflhip_rotate_hoisted_level_ntt_dev(e.ctx, p0, p1, a0.data_ptr(), a1.data_ptr(), pk, kv, 2, 3, 2, 2, level, flags, sp)

            def lt():
                return _lib.lib.nflhip_lintrans_level_ntt_dev(e.ctx, o[0, 0].data_ptr(), o[0, 1].data_ptr(), a0.data_ptr(), a1.data_ptr(), pk, pw, kv,
                                                              2, 3, 2, 2, level, flags, sp)
            for call in (rot, lt):
                o.fill_(5)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.stream(st):
                    with torch.cuda.graph(g, stream=st):
                        z.add_(1)
                        rc = call()
                torch.cuda.synchronize()
                assert rc == _lib.ERR_UNSUPPORTED, (level, flags, rc)
                assert bool((o == 5).all())                                  # nothing was enqueued
                assert call() == 0                                          # the same stream
                st.synchronize()
                if level == 3 and call is rot:
                    assert same_rot(e, [(o[0, 0], o[0, 1]), (o[1, 0], o[1, 1])], wr), flags
                elif level == 3:
                    assert same_lt(e, (o[0, 0], o[0, 1]), wl), flags
    finally:
        e.close()


def test_invalid_arguments(engine_factory, oracle_factory):
    """levels 0, L + 1 and 2^64 - 1; an output over the live part of a key, over an input, over a weight: NFLHIP_ERR_INVALID, nothing
    written.  An output over the DEAD digits of a key is no overlap."""
    import torch
    from nfllib_amd import _lib
    e, c0, c1, keys, ws, want_rot, want_lt = _shared(engine_factory, oracle_factory)
    ks, which = rotations(64, 2)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:2]]
    o = torch.zeros((2, 2) + c1.shape, dtype=torch.int64, device="cuda:0")
    kv = (C.c_uint64 * 2)(*ks)
    rot, lt = _lib.lib.nflhip_rotate_hoisted_level_ntt_dev, _lib.lib.nflhip_lintrans_level_ntt_dev

    def arr(xs):
        return (C.c_void_p * len(xs))(*xs)

    def call_rot(level=3, o0=None, o1=None, c0p=dc0.data_ptr(), keys_=None, count=2):
        return rot(e.ctx, arr(o0 or [o[0, 0].data_ptr(), o[1, 0].data_ptr()]), arr(o1 or [o[0, 1].data_ptr(), o[1, 1].data_ptr()]), c0p, dc1.data_ptr(),
                   arr(keys_ or [dkeys[i].data_ptr() for i in which]), kv, count, 3, 2, 2, level, 0, None)

    def call_lt(level=3, o0=o[0, 0].data_ptr(), o1=o[0, 1].data_ptr(), keys_=None, ws_=None, count=2):
        return lt(e.ctx, o0, o1, dc0.data_ptr(), dc1.data_ptr(), arr(keys_ or [dkeys[i].data_ptr() for i in which]),
                  arr(ws_ or [w.data_ptr() for w in dws]), kv, count, 3, 2, 2, level, 0, None)
    bad = _lib.ERR_INVALID
    for level in (0, 5, 2**64 - 1):
        assert call_rot(level=level) == bad and call_lt(level=level) == bad
    assert call_rot(count=0) == bad and call_rot(count=17) == bad and call_lt(count=0) == bad and call_lt(count=17) == bad
    key0 = dkeys[0]                                                           # [2 digits][2][6][64] at the top; level 3 reads both digits
    assert call_rot(o0=[key0[1, 1, 3].data_ptr(), o[1, 0].data_ptr()]) == bad       # inside the live digits
    assert call_lt(o1=key0[0, 0].data_ptr()) == bad
    assert call_rot(o0=[dc1.data_ptr(), o[1, 0].data_ptr()]) == bad and call_lt(o0=dc0.data_ptr()) == bad
    assert call_lt(o0=dws[1][3:].data_ptr()) == bad                           # a weight is a whole polynomial of the context at every level
    assert call_rot(o1=[o[0, 0].data_ptr(), o[1, 1].data_ptr()]) == bad       # two outputs overlap
    torch.cuda.synchronize()
    assert bool((o == 0).all()) and np.array_equal(e.to_host(key0), keys[0]) and np.array_equal(e.to_host(dc1), c1)
    # level 1 reads one digit of two: an output in the second digit of a (scratch copy of a) key does not overlap its live extent
    b0, b1, _, _, want1, _ = case(e, oracle_factory(64, 64, 6), 2, 2, 1)
    a0, a1 = e.to_device(b0), e.to_device(b1)
    k = key0.clone()
    out = k[1].reshape(-1)[:4 * 3 * 64].view(2, 2, 3, 1, 64)                  # 768 of the second digit's 768 words
    rc = rot(e.ctx, arr([out[0, 0].data_ptr(), out[1, 0].data_ptr()]), arr([out[0, 1].data_ptr(), out[1, 1].data_ptr()]), a0.data_ptr(), a1.data_ptr(),
             arr([k.data_ptr(), dkeys[1].data_ptr()]), kv, 2, 3, 2, 2, 1, 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert same_rot(e, [(out[0, 0], out[0, 1]), (out[1, 0], out[1, 1])], want1(False, False, ks, which))


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_level_rotate_cpp import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_level_rotate")), gpu=True)


@pytest.mark.parametrize("batch", [1, 5])
def test_cpp_surface_on_the_gpu(cpp_program, batch):
    """the program of tests/cpp_level_rotate against the real library: poly, poly_p and device_batch equal to the C entries on raw
    pointers with K, the level, the whole keys and the whole diagonals written out, and at the top level to the existing header calls"""
    import os
    import subprocess
    r = subprocess.run([cpp_program, str(batch)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
