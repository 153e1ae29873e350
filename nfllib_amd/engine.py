"""Host-side driver of the HIP engine for tests, bench.py and the multi-GPU
batch split.  This is plumbing over the C ABI (include/nflhip.h): device
memory and streams come from PyTorch, all arithmetic happens in libnflhip.so.

Data layout is the reference's: a batch of nfl::poly<T,Degree,NbModuli> is a
dense [batch][NbModuli][Degree] tensor of T (poly.hpp:82-88, tests/tools.h:6-17).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (SCALE_ROUND_FLOOR, SCALE_ROUND_KEEP, SCALE_ROUND_TWO_PASS, MULRELIN_CENTERED, MULRELIN_FLOOR, MULRELIN_FUSED, MULRELIN_MERGED, MULRELIN_RESCALE, MULRELIN_SEQUENCE, LINTRANS_CENTERED, LINTRANS_FLOOR, LINTRANS_HOISTED, LINTRANS_MAX_TERMS, LINTRANS_SEQUENCE, MAC_MAX_TERMS, MAC_DOUBLE_BUFFER, MAC_MULTI_MAX_OUTPUTS, BSGS_CENTERED, BSGS_FLOOR, BSGS_HOISTED, BSGS_MAX_BABY, BSGS_MAX_GIANT, BSGS_SEQUENCE, DOT_MULTI_MAX_OUTPUTS, ROTATE_CENTERED, ROTATE_FLOOR, ROTATE_HOISTED, ROTATE_MAX_OUTPUTS, ROTATE_SEQUENCE, KEYSWITCH_CENTERED, KEYSWITCH_COMPOSED, KEYSWITCH_FLOOR, KEYSWITCH_FUSED, KEYSWITCH_SEQUENCE, AUTOMORPHISM_MAX_OUTPUTS, BASECONV_CENTERED, BASECONV_NTT_COMPOSED, BASECONV_NTT_FUSED, MODDOWN_FLOOR, DECOMP_COMPOSED, DECOMP_FUSED, DECOMP_SIGNED, DOT_MAX_POINTERS, DOT_UNTILED, FORM_COEFF, FORM_NTT, RESCALE_COMPOSED, RESCALE_FUSED,  # noqa: F401
                   FMT_I8, FMT_I16, FMT_I32, FMT_WORDS, NflHipError, OP_ADD, OP_COMPUTE_SHOUP, OP_MUL, OP_MUL_SHOUP, OP_SUB,  # noqa: F401
                   DIST_REFERENCE_WORDS, ROW_BITREV_IO, ROW_INVERSE_TABLES, TAB_INVDEGREE, TAB_INVOMEGAS,
                   TAB_INVPOLY_INVPHIS, TAB_MODULUS, TAB_OMEGAS, TAB_PHIS, TAB_PSI, TAB_SHOUPINVPOLY_INVPHIS,
                   TAB_SHOUPPHIS)
from .params import params as limb_params

_NP = {16: np.uint16, 32: np.uint32, 64: np.uint64}


def _torch():
    import torch
    return torch


def _vp(x):
    """void* of a numpy array, a torch tensor, an int or None."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if isinstance(x, int):
        return C.c_void_p(x)
    return C.c_void_p(x.data_ptr())


DIST_UNIFORM, DIST_BOUNDED, DIST_ZO, DIST_HWT = 0, 1, 2, 3   # NFLHIP_DIST_* (include/nflhip.h)


class Engine:
    """One (T, Degree, NbModuli) context on one GPU -- the device-side
    counterpart of poly<T,Degree,NbModuli>::base / ::gmp (poly.hpp:247, 275)."""

    def __init__(self, limb_bits, degree, nmoduli, device=0, rows=None):
        """the context over the first nmoduli moduli of the limb width; rows = a list of nmoduli distinct modulus indices: over
        those moduli instead, in that order (level_engine)"""
        self.lib = _lib.lib
        self.limb_bits, self.degree, self.nmoduli, self.device = limb_bits, degree, nmoduli, device
        self.np_dtype = np.dtype(_NP[limb_bits])
        pr = self.params = limb_params(limb_bits)
        rows = list(range(nmoduli)) if rows is None else [int(r) for r in rows]
        if nmoduli > pr.max_moduli:
            raise ValueError("only %d moduli are mirrored for %d-bit limbs" % (pr.max_moduli, limb_bits))
        if len(rows) != nmoduli or len(set(rows)) != nmoduli or not all(0 <= r < pr.max_moduli for r in rows):
            raise ValueError("rows are nmoduli = %d distinct modulus indices below %d" % (nmoduli, pr.max_moduli))
        self.rows = rows
        self._keep = [np.ascontiguousarray(x[rows]) for x in (pr.P, pr.primitive_roots, pr.invkmax)]
        h = C.c_void_p()
        rc = self.lib.nflhip_ctx_create(C.byref(h), device, limb_bits, degree, nmoduli,
                                        *[_vp(x) for x in self._keep], pr.kmax_log2)
        if rc != 0:
            raise NflHipError(rc, self.lib.nflhip_last_error(None).decode())
        self.ctx = h
        self.P = [int(v) for v in self._keep[0]]
        self.crt_limbs = self.lib.nflhip_crt_limbs(self.ctx)
        self.words_per_poly = degree * nmoduli
        self._next_stream = 1 << 32   # ids handed out to sampler calls that do not name one (see _sid)
        self.bytes_per_poly = self.words_per_poly * self.np_dtype.itemsize

    def close(self):
        kept = self.__dict__.pop("_bfv_kept", None)   # (bfv_mul_relin_ntt's engine over the first L moduli)
        if kept is not None:
            kept.close()
        if getattr(self, "ctx", None):
            self.lib.nflhip_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise NflHipError(rc, self.lib.nflhip_last_error(self.ctx).decode())

    # ---- device tensors (torch is only the allocator / stream provider) ----
    @property
    def torch_dtype(self):
        t = _torch()
        return {16: t.int16, 32: t.int32, 64: t.int64}[self.limb_bits]

    def empty(self, batch):
        t = _torch()
        return t.empty((batch, self.nmoduli, self.degree), dtype=self.torch_dtype, device="cuda:%d" % self.device)

    def to_device(self, arr):
        t = _torch()
        arr = np.ascontiguousarray(arr, dtype=self.np_dtype)
        signed = arr.view({16: np.int16, 32: np.int32, 64: np.int64}[self.limb_bits])
        return t.from_numpy(signed.copy()).to("cuda:%d" % self.device)

    def to_host(self, ten):
        return ten.detach().cpu().contiguous().numpy().view(self.np_dtype)

    def _stream(self, stream=None):
        t = _torch()
        s = stream if stream is not None else t.cuda.current_stream(self.device)
        return C.c_void_p(s.cuda_stream)

    def _batch(self, ten):
        n = ten.numel()
        assert n % self.words_per_poly == 0 and ten.is_contiguous()
        return n // self.words_per_poly

    def ntt_(self, d, stream=None):
        self._chk(self.lib.nflhip_ntt_fwd_dev(self.ctx, _vp(d), self._batch(d), self._stream(stream)))
        return d

    def intt_(self, d, stream=None):
        self._chk(self.lib.nflhip_ntt_inv_dev(self.ctx, _vp(d), self._batch(d), self._stream(stream)))
        return d

    def ntt_row_(self, rows, cm, inverse_tables=False, bitrev_io=False, stream=None):
        """core::ntt (core.hpp:455-532) on contiguous rows of modulus cm, in place: cyclic, natural in, bit-reversed
        out; inverse_tables selects the invomegas tables, bitrev_io wraps it in the two permutations of core::inv_ntt"""
        assert rows.is_contiguous() and rows.numel() % self.degree == 0
        mode = (ROW_INVERSE_TABLES if inverse_tables else 0) | (ROW_BITREV_IO if bitrev_io else 0)
        self._chk(self.lib.nflhip_ntt_row_dev(self.ctx, _vp(rows), cm, mode, rows.numel() // self.degree,
                                              self._stream(stream)))
        return rows

    def h_ntt_row(self, rows, cm, inverse_tables=False, bitrev_io=False):
        out = np.ascontiguousarray(rows, dtype=self.np_dtype).copy()
        mode = (ROW_INVERSE_TABLES if inverse_tables else 0) | (ROW_BITREV_IO if bitrev_io else 0)
        self._chk(self.lib.nflhip_ntt_row(self.ctx, _vp(out), cm, mode, out.size // self.degree))
        return out

    # ---- Galois automorphisms sigma_k : a(X) -> a(X^k) mod (X^n + 1), k odd (include/nflhip.h "Galois automorphisms") ----
    def _k(self, k):
        """k reduced mod 2n (a negative k names the same automorphism as k mod 2n)"""
        return int(k) % (2 * self.degree)

    def automorphism(self, d, k, ntt=False, out=None, stream=None):
        """sigma_k of every polynomial of d (coefficient form, or NTT form with ntt=True) into a new tensor or `out`,
        which must not overlap d"""
        out = out if out is not None else _torch().empty_like(d)
        form = FORM_NTT if ntt else FORM_COEFF
        self._chk(self.lib.nflhip_automorphism_dev(self.ctx, _vp(out), _vp(d), self._batch(d), self._k(k), form,
                                                   self._stream(stream)))
        return out

    def automorphism_multi(self, d, ks, ntt=False, outs=None, stream=None):
        """[sigma_k(d) for k in ks] in ONE launch that reads d once (at most 16 multipliers)"""
        ks = [self._k(k) for k in ks]
        outs = list(outs) if outs is not None else [_torch().empty_like(d) for _ in ks]
        ptrs = (C.c_void_p * max(len(outs), 1))(*[o.data_ptr() for o in outs])
        kv = (C.c_uint64 * max(len(ks), 1))(*ks)
        form = FORM_NTT if ntt else FORM_COEFF
        self._chk(self.lib.nflhip_automorphism_multi_dev(self.ctx, ptrs, kv, len(ks), _vp(d), self._batch(d), form,
                                                         self._stream(stream)))
        return outs

    def h_automorphism(self, a, k, ntt=False):
        """host-pointer variant: sigma_k of a numpy batch, staged through the context (nflhip_automorphism)"""
        out = np.empty_like(a)
        form = FORM_NTT if ntt else FORM_COEFF
        self._chk(self.lib.nflhip_automorphism(self.ctx, _vp(out), _vp(a), self._hb(a), self._k(k), form))
        return out

    # ---- RNS rescale: divide and round by the last modulus (include/nflhip.h "RNS rescale") ----
    def rescale(self, d, ntt=False, out=None, stream=None, composed=False, fused=False):
        """floor((X + h) / q) of every coefficient, q the last modulus: [batch, nm, n] -> a new [batch, nm - 1, n] tensor
        (or `out`, which must not overlap d) in the layout of Engine(limb_bits, degree, nm - 1); ntt=True for NTT-form
        data; composed=True / fused=True force the composed NTT-form plan / the one-launch kernel"""
        batch = self._batch(d)
        if out is None:
            out = _torch().empty((batch, self.nmoduli - 1, self.degree), dtype=self.torch_dtype, device=d.device)
        form = (FORM_NTT | (RESCALE_COMPOSED if composed else 0) | (RESCALE_FUSED if fused else 0)) if ntt else FORM_COEFF
        self._chk(self.lib.nflhip_rescale_dev(self.ctx, _vp(out), _vp(d), batch, form, self._stream(stream)))
        return out

    def h_rescale(self, a, ntt=False):
        """host-pointer variant: a numpy [batch, nm, n] batch -> [batch, nm - 1, n], staged through the context"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        batch = self._hb(a)
        out = np.empty((batch, self.nmoduli - 1, self.degree), dtype=self.np_dtype)
        self._chk(self.lib.nflhip_rescale(self.ctx, _vp(out), _vp(a), batch, FORM_NTT if ntt else FORM_COEFF))
        return out

    # ---- sums of products across polynomials (include/nflhip.h "sums of products") ----
    def dot_strided(self, a, a_strides, b, b_strides, groups, terms, addend=None, out=None, untiled=False, stream=None):
        """out[g] = addend[g] + sum_j a(g, j) * b(g, j): polynomial (g, j) of an operand starts g * strides[0] + j * strides[1]
        polynomials after its first word (strides[0] == 0: shared by all groups); a / b are tensors (views allowed) or device
        addresses; addend may be `out` itself; untiled=True forces one group per pass where an operand is shared"""
        if out is None:
            out = self.empty(groups)
        oa = _lib.DotOperand(a if isinstance(a, int) else a.data_ptr(), a_strides[0], a_strides[1])
        ob = _lib.DotOperand(b if isinstance(b, int) else b.data_ptr(), b_strides[0], b_strides[1])
        self._chk(self.lib.nflhip_dot_dev(self.ctx, _vp(out), C.byref(oa), C.byref(ob), _vp(addend), groups, terms,
                                          DOT_UNTILED if untiled else 0, self._stream(stream)))
        return out

    def dot(self, a, b, terms, addend=None, out=None, untiled=False, stream=None):
        """a and b dense with groups * terms polynomials: out[g] = addend[g] + sum_j a[g * terms + j] * b[g * terms + j]"""
        batch = self._batch(a)
        if terms <= 0 or batch % terms or self._batch(b) != batch:
            raise ValueError("a and b hold groups * terms polynomials each")
        return self.dot_strided(a, (terms, 1), b, (terms, 1), batch // terms, terms, addend, out, untiled, stream)

    def matvec(self, m, v, addend=None, out=None, untiled=False, stream=None):
        """matrix times shared vector: v holds `terms` polynomials, m groups * terms: out[g] = addend[g] + sum_j m[g, j] * v[j]"""
        terms, batch = self._batch(v), self._batch(m)
        if terms == 0 or batch % terms:
            raise ValueError("m holds groups * terms polynomials, v terms")
        return self.dot_strided(m, (terms, 1), v, (0, 1), batch // terms, terms, addend, out, untiled, stream)

    def dot_list(self, as_, bs, addend=None, out=None, stream=None):
        """one polynomial: addend + sum_j as_[j] * bs[j] over lists of one-polynomial tensors anywhere in device memory; the
        pointers travel by value, 16 per launch, longer lists chain through the addend"""
        if len(as_) != len(bs) or not as_:
            raise ValueError("two lists of one length, at least one term")
        if out is None:
            out = self.empty(1)
        for k in range(0, len(as_), DOT_MAX_POINTERS):
            xa, xb = as_[k:k + DOT_MAX_POINTERS], bs[k:k + DOT_MAX_POINTERS]
            pa = (C.c_void_p * len(xa))(*[x.data_ptr() for x in xa])
            pb = (C.c_void_p * len(xb))(*[x.data_ptr() for x in xb])
            self._chk(self.lib.nflhip_dot_ptrs_dev(self.ctx, _vp(out), pa, pb, len(xa), _vp(addend if k == 0 else out),
                                                   self._stream(stream)))
        return out

    def dot_multi(self, a, a_strides, bs, b_term_stride, groups, terms, outs=None, untiled=False, stream=None):
        """outs[o][g] = sum_j a(g, j) * bs[o](j) for every o in ONE launch that reads `a` once (at most 32 outputs): polynomial (g, j)
        of a starts g * a_strides[0] + j * a_strides[1] polynomials after its first word, term j of bs[o] j * b_term_stride after
        its first word, shared by every group; a and every bs[o] are tensors (views allowed) or device addresses.  Returns the
        list of dense [groups, nm, n] tensors; untiled=True forces one group per pass"""
        bs = list(bs)
        outs = list(outs) if outs is not None else [self.empty(groups) for _ in bs]
        if len(outs) != len(bs):
            raise ValueError("one output per second operand")
        oa = _lib.DotOperand(a if isinstance(a, int) else a.data_ptr(), a_strides[0], a_strides[1])
        po = (C.c_void_p * max(len(outs), 1))(*[o if isinstance(o, int) else o.data_ptr() for o in outs])
        pb = (C.c_void_p * max(len(bs), 1))(*[b if isinstance(b, int) else b.data_ptr() for b in bs])
        self._chk(self.lib.nflhip_dot_multi_dev(self.ctx, po, C.byref(oa), pb, b_term_stride, len(bs), groups, terms,
                                                DOT_UNTILED if untiled else 0, self._stream(stream)))
        return outs

    def h_dot(self, a, b, terms, b_shared=False):
        """host-pointer variant: numpy a = [groups * terms, nm, n], b alike or [terms, nm, n] with b_shared; -> [groups, nm, n]"""
        a, b = np.ascontiguousarray(a, dtype=self.np_dtype), np.ascontiguousarray(b, dtype=self.np_dtype)
        if terms <= 0 or self._hb(a) % terms or self._hb(b) != (terms if b_shared else self._hb(a)):
            raise ValueError("a holds groups * terms polynomials, b as many, or terms with b_shared")
        groups = self._hb(a) // terms
        out = np.empty((groups, self.nmoduli, self.degree), dtype=self.np_dtype)
        self._chk(self.lib.nflhip_dot(self.ctx, _vp(out), _vp(a), _vp(b), groups, terms, int(bool(b_shared))))
        return out

    # ---- gadget decomposition: base-2^w digits of RNS rows (include/nflhip.h "gadget decomposition") ----
    _DECOMP_FMT = {"words": FMT_WORDS, "i8": FMT_I8, "i16": FMT_I16, "i32": FMT_I32}

    def decompose_terms(self, w):
        """nmoduli * ceil(modulus bits / w) digit polynomials per input polynomial"""
        terms = self.lib.nflhip_decompose_terms(self.ctx, w)
        if terms == 0:
            raise ValueError("digit width %r is out of range (1 to %d)" % (w, self.limb_bits - 3))
        return terms

    def _decomp_flags(self, signed, ntt, plan):
        if plan not in (None, "composed", "fused"):
            raise ValueError("plan is None, 'composed' or 'fused'")
        return ((FORM_NTT if ntt else FORM_COEFF) | (DECOMP_SIGNED if signed else 0) |
                {None: 0, "composed": DECOMP_COMPOSED, "fused": DECOMP_FUSED}[plan])

    def decompose(self, a, w, signed=False, ntt=False, fmt="words", out=None, plan=None, stream=None):
        """the base-2^w digits of every row of the coefficient-form batch a = [batch, nm, n]: term j = m * l + t is digit t of row m.
        fmt "words" -> [batch * terms, nm, n], the digit spread over every row (ntt=True: forward-transformed; plan "composed" /
        "fused" forces a plan); fmt "i8" / "i16" / "i32" -> [batch * terms, n] signed integers.  signed=True: balanced digits."""
        t = _torch()
        batch, terms, f = self._batch(a), self.decompose_terms(w), self._DECOMP_FMT[fmt]
        if out is None:
            if f == FMT_WORDS:
                out = t.empty((batch * terms, self.nmoduli, self.degree), dtype=self.torch_dtype, device=a.device)
            else:
                out = t.empty((batch * terms, self.degree), dtype={FMT_I8: t.int8, FMT_I16: t.int16, FMT_I32: t.int32}[f], device=a.device)
        self._chk(self.lib.nflhip_decompose_dev(self.ctx, _vp(out), f, _vp(a), batch, w, self._decomp_flags(signed, ntt, plan),
                                                self._stream(stream)))
        return out

    def h_decompose(self, a, w, signed=False, ntt=False, fmt="words"):
        """host-pointer variant: a numpy [batch, nm, n] batch -> [batch * terms, nm, n] words or [batch * terms, n] integers"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        batch, terms, f = self._hb(a), self.decompose_terms(w), self._DECOMP_FMT[fmt]
        if f == FMT_WORDS:
            out = np.empty((batch * terms, self.nmoduli, self.degree), dtype=self.np_dtype)
        else:
            out = np.empty((batch * terms, self.degree), dtype={FMT_I8: np.int8, FMT_I16: np.int16, FMT_I32: np.int32}[f])
        self._chk(self.lib.nflhip_decompose(self.ctx, _vp(out), f, _vp(a), batch, w, self._decomp_flags(signed, ntt, None)))
        return out

    def gadget_mul(self, a, w, out=None, stream=None):
        """key-generation companion: [batch, nm, n] -> [batch * terms, nm, n], term (m, t) holds a[m] * 2^(w t) mod p_m in row m and
        zeros elsewhere, so that sum_j decompose(x)[j] * gadget_mul(y)[j] = x * y in every row"""
        batch, terms = self._batch(a), self.decompose_terms(w)
        if out is None:
            out = _torch().empty((batch * terms, self.nmoduli, self.degree), dtype=self.torch_dtype, device=a.device)
        self._chk(self.lib.nflhip_gadget_mul_dev(self.ctx, _vp(out), _vp(a), batch, w, self._stream(stream)))
        return out

    # ---- RNS base conversion and mod-down by the last k moduli (include/nflhip.h "RNS base conversion") ----
    def baseconv(self, a, src, dst, centered=False, out=None, stream=None):
        """rows src = (first, count) of the coefficient-form batch a = [batch, nm, n] converted to rows dst = (first, count): the
        fast conversion x + u Q, or with centered=True the centred representative of x.  out=None works in place on a (the
        normal mod-up); another `out` = [batch, nm, n] must not overlap a, and only its rows dst are written.  The first call
        for a pair of ranges uploads its tables: make it before a graph capture."""
        out = a if out is None else out
        self._chk(self.lib.nflhip_baseconv_dev(self.ctx, _vp(out), _vp(a), self._batch(a), src[0], src[1], dst[0], dst[1],
                                               BASECONV_CENTERED if centered else 0, self._stream(stream)))
        return out

    def mod_up(self, a, src, stream=None):
        """baseconv from rows src = (first, count) to every row, in place (the source rows keep their words)"""
        return self.baseconv(a, src, (0, self.nmoduli), stream=stream)

    def mod_down(self, a, k, floor=False, out=None, stream=None):
        """X / P rounded to nearest, P the product of the last k moduli (floor=True: floor(X / P) - u, the approximate mod-down):
        [batch, nm, n] -> a new [batch, nm - k, n] tensor (or `out`, which must not overlap a) in the layout of
        Engine(limb_bits, degree, nm - k); coefficient form"""
        batch = self._batch(a)
        if out is None:
            out = _torch().empty((batch, max(self.nmoduli - k, 0), self.degree), dtype=self.torch_dtype, device=a.device)
        self._chk(self.lib.nflhip_moddown_dev(self.ctx, _vp(out), _vp(a), batch, k, MODDOWN_FLOOR if floor else 0, self._stream(stream)))
        return out

    def h_baseconv(self, a, src, dst, centered=False):
        """host-pointer variant: a numpy [batch, nm, n] batch -> a new one with rows dst converted from rows src"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        out = np.empty_like(a)
        self._chk(self.lib.nflhip_baseconv(self.ctx, _vp(out), _vp(a), self._hb(a), src[0], src[1], dst[0], dst[1],
                                           BASECONV_CENTERED if centered else 0))
        return out

    def h_mod_down(self, a, k, floor=False):
        """host-pointer variant: a numpy [batch, nm, n] batch -> [batch, nm - k, n]"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        batch = self._hb(a)
        out = np.empty((batch, max(self.nmoduli - k, 0), self.degree), dtype=self.np_dtype)
        self._chk(self.lib.nflhip_moddown(self.ctx, _vp(out), _vp(a), batch, k, MODDOWN_FLOOR if floor else 0))
        return out

    # ---- the same on NTT-form data (include/nflhip.h "RNS base conversion and mod-down, NTT form") ----
    _BCN_PLAN = {None: 0, "composed": BASECONV_NTT_COMPOSED, "fused": BASECONV_NTT_FUSED}

    def baseconv_ntt(self, a, src, dst, centered=False, out=None, plan=None, stream=None):
        """baseconv on the NTT-form batch a: every written row is the forward transform of what baseconv writes for the
        coefficient form of a.  out=None works in place on a; plan="fused" / "composed" forces the one-launch kernel / the composed
        plan.  The first call for a pair of ranges (and, composed, for a larger batch) allocates: make it before a graph capture."""
        out = a if out is None else out
        flags = (BASECONV_CENTERED if centered else 0) | self._BCN_PLAN[plan]
        self._chk(self.lib.nflhip_baseconv_ntt_dev(self.ctx, _vp(out), _vp(a), self._batch(a), src[0], src[1], dst[0], dst[1], flags,
                                                   self._stream(stream)))
        return out

    def mod_up_ntt(self, a, src, centered=False, plan=None, stream=None):
        """baseconv_ntt from rows src = (first, count) to every row, in place (the source rows keep their words)"""
        return self.baseconv_ntt(a, src, (0, self.nmoduli), centered=centered, plan=plan, stream=stream)

    def mod_down_ntt(self, a, k, floor=False, out=None, plan=None, stream=None):
        """mod_down on the NTT-form batch a: [batch, nm, n] -> a new [batch, nm - k, n] tensor (or `out`, which must not overlap a),
        NTT form in the layout of Engine(limb_bits, degree, nm - k)"""
        batch = self._batch(a)
        if out is None:
            out = _torch().empty((batch, max(self.nmoduli - k, 0), self.degree), dtype=self.torch_dtype, device=a.device)
        flags = (MODDOWN_FLOOR if floor else 0) | self._BCN_PLAN[plan]
        self._chk(self.lib.nflhip_moddown_ntt_dev(self.ctx, _vp(out), _vp(a), batch, k, flags, self._stream(stream)))
        return out

    def h_baseconv_ntt(self, a, src, dst, centered=False, plan=None):
        """host-pointer variant: a numpy NTT-form [batch, nm, n] batch -> a new one with rows dst converted from rows src"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        out = np.empty_like(a)
        self._chk(self.lib.nflhip_baseconv_ntt(self.ctx, _vp(out), _vp(a), self._hb(a), src[0], src[1], dst[0], dst[1],
                                               (BASECONV_CENTERED if centered else 0) | self._BCN_PLAN[plan]))
        return out

    def h_mod_down_ntt(self, a, k, floor=False, plan=None):
        """host-pointer variant: a numpy NTT-form [batch, nm, n] batch -> [batch, nm - k, n]"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        batch = self._hb(a)
        out = np.empty((batch, max(self.nmoduli - k, 0), self.degree), dtype=self.np_dtype)
        self._chk(self.lib.nflhip_moddown_ntt(self.ctx, _vp(out), _vp(a), batch, k, (MODDOWN_FLOOR if floor else 0) | self._BCN_PLAN[plan]))
        return out

    # ---- hybrid key switching, NTT form (include/nflhip.h "hybrid key switching") ----
    _KS_PLAN = {None: 0, "sequence": KEYSWITCH_SEQUENCE, "composed": KEYSWITCH_COMPOSED, "fused": KEYSWITCH_FUSED}

    def keyswitch_digits(self, k_special, alpha, level=None):
        """dnum = ceil((nm - k_special) / alpha), the number of digits (and of key terms) of a key switch; with a level,
        ceil(level / alpha): the digits a call at that level reads"""
        if level is not None:
            dnum = self.lib.nflhip_keyswitch_level_digits(self.ctx, k_special, alpha, level)
            if dnum == 0:
                raise ValueError("k_special %r (1 to nm - 1), alpha %r (1 to nm - k_special) or level %r (1 to nm - k_special) is out of range"
                                 % (k_special, alpha, level))
            return dnum
        dnum = self.lib.nflhip_keyswitch_digits(self.ctx, k_special, alpha)
        if dnum == 0:
            raise ValueError("k_special %r (1 to nm - 1) or alpha %r (1 to nm - k_special) is out of range" % (k_special, alpha))
        return dnum

    def level_rows(self, level, k_special):
        """A_l: the rows of this context that are alive at a level, [0, level) and the k_special special rows"""
        L = self.nmoduli - k_special
        if k_special < 1 or L < 1 or not 1 <= level <= L:
            raise ValueError("k_special is 1 to nm - 1, level 1 to nm - k_special")
        return list(range(level)) + list(range(L, self.nmoduli))

    def level_engine(self, level, k_special):
        """an Engine over C_l, the moduli of level_rows(level, k_special) in that order, on the same device: a call with level=l on
        this engine returns the words of the same call on that engine with key[:dnum_l, :, level_rows] -- the definition of a level
        call, and how test vectors for one are prepared"""
        rows = [self.rows[r] for r in self.level_rows(level, k_special)]
        return Engine(self.limb_bits, self.degree, len(rows), device=self.device, rows=rows)

    def _level_key(self, size, k_special, alpha, level):
        """a key for a call at a level: the whole [dnum_L, 2, nm, n], or as many leading digits as the level reads, at least"""
        lo, hi = self.keyswitch_digits(k_special, alpha, level), self.keyswitch_digits(k_special, alpha)
        if size % (2 * self.words_per_poly) or not lo <= size // (2 * self.words_per_poly) <= hi:
            raise ValueError("key holds dnum * 2 polynomials of this context (the digits of the level, at least)")

    def _ks_flags(self, centered, floor, plan):
        return (KEYSWITCH_CENTERED if centered else 0) | (KEYSWITCH_FLOOR if floor else 0) | self._KS_PLAN[plan]

    def key_switch_ntt(self, a, key, k_special, alpha, centered=False, floor=False, out=None, plan=None, stream=None, level=None):
        """the hybrid key switch of the NTT-form batch a = [batch, L, n], L = nm - k_special (the layout of Engine(limb_bits, degree, L)),
        against key = [dnum, 2, nm, n] (NTT form over this context, shared by the batch): mod-up of every digit of alpha rows (fast,
        or centered=True), the two sums of products, mod-down by the last k_special moduli (rounding, or floor=True).  Returns
        (out0, out1), each [batch, L, n]; `out` = a pair of such tensors, else both are views of one new [2, batch, L, n] tensor.
        plan "sequence" / "composed" / "fused" forces a plan.  The first call for a (k_special, alpha), or a larger batch,
        allocates: make it before a graph capture.
        level=l (1 to L): a and the results are [batch, l, n], a ciphertext below the top level, and the key is still the ONE
        top-level key, of which only the live rows [0, l), [L, nm) and the first ceil(l / alpha) digits are read."""
        if level is not None:
            return self._key_switch_level(a, key, k_special, alpha, level, self._ks_flags(centered, floor, plan), out, stream)
        L = self.nmoduli - k_special
        if L <= 0 or a.numel() % (L * self.degree) or not a.is_contiguous() or not key.is_contiguous():
            raise ValueError("a is a contiguous [batch, nm - k_special, n] tensor")
        batch = a.numel() // (L * self.degree)
        if key.numel() != 2 * self.keyswitch_digits(k_special, alpha) * self.words_per_poly:
            raise ValueError("key holds dnum * 2 polynomials of this context")
        if out is None:
            both = _torch().empty((2, batch, L, self.degree), dtype=self.torch_dtype, device=a.device)
            out = (both[0], both[1])
        self._chk(self.lib.nflhip_keyswitch_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(a), _vp(key), batch, k_special, alpha,
                                                    self._ks_flags(centered, floor, plan), self._stream(stream)))
        return out

    def _key_switch_level(self, a, key, k_special, alpha, level, flags, out, stream):
        self.level_rows(level, k_special)
        if a.numel() % (level * self.degree) or not a.is_contiguous() or not key.is_contiguous():
            raise ValueError("a is a contiguous [batch, level, n] tensor")
        batch = a.numel() // (level * self.degree)
        self._level_key(key.numel(), k_special, alpha, level)
        if out is None:
            both = _torch().empty((2, batch, level, self.degree), dtype=self.torch_dtype, device=a.device)
            out = (both[0], both[1])
        self._chk(self.lib.nflhip_keyswitch_level_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(a), _vp(key), batch, k_special, alpha, level,
                                                          flags, self._stream(stream)))
        return out

    def h_key_switch_ntt(self, a, key, k_special, alpha, centered=False, floor=False, plan=None, level=None):
        """host-pointer variant: numpy a = [batch, L, n] and key = [dnum, 2, nm, n] -> (out0, out1); level as key_switch_ntt"""
        a, key = np.ascontiguousarray(a, dtype=self.np_dtype), np.ascontiguousarray(key, dtype=self.np_dtype)
        if level is not None:
            self.level_rows(level, k_special)
            if a.size % (level * self.degree):
                raise ValueError("a is [batch, level, n]")
            self._level_key(key.size, k_special, alpha, level)
            batch = a.size // (level * self.degree)
            out0, out1 = (np.empty((batch, level, self.degree), dtype=self.np_dtype) for _ in range(2))
            self._chk(self.lib.nflhip_keyswitch_level_ntt(self.ctx, _vp(out0), _vp(out1), _vp(a), _vp(key), batch, k_special, alpha, level,
                                                          self._ks_flags(centered, floor, plan)))
            return out0, out1
        L = self.nmoduli - k_special
        if L <= 0 or a.size % (L * self.degree) or key.size != 2 * self.keyswitch_digits(k_special, alpha) * self.words_per_poly:
            raise ValueError("a is [batch, nm - k_special, n], key [dnum, 2, nm, n]")
        batch = a.size // (L * self.degree)
        out0, out1 = (np.empty((batch, L, self.degree), dtype=self.np_dtype) for _ in range(2))
        self._chk(self.lib.nflhip_keyswitch_ntt(self.ctx, _vp(out0), _vp(out1), _vp(a), _vp(key), batch, k_special, alpha,
                                                self._ks_flags(centered, floor, plan)))
        return out0, out1

    # ---- hoisted rotations: one mod-up shared by many Galois key switches (include/nflhip.h "hoisted rotations") ----
    _ROT_PLAN = {None: 0, "sequence": ROTATE_SEQUENCE, "hoisted": ROTATE_HOISTED}

    def _rot_flags(self, centered, floor, plan):
        return (ROTATE_CENTERED if centered else 0) | (ROTATE_FLOOR if floor else 0) | self._ROT_PLAN[plan]

    def _level_keys(self, keys, size, k_special, alpha, level):
        """the key check of a call over several keys: whole keys of this context at the top level (level None), _level_key below it"""
        if level is None:
            kwords = 2 * self.keyswitch_digits(k_special, alpha) * self.words_per_poly
            return all(k is None or size(k) == kwords for k in keys)
        for k in keys:
            if k is not None:
                self._level_key(size(k), k_special, alpha, level)
        return True

    def rotate_hoisted_ntt(self, c0, c1, keys, ks, k_special, alpha, centered=False, floor=False, outs=None, plan=None, stream=None, level=None):
        """the ciphertext (c0, c1), each an NTT-form [batch, L, n] batch with L = nm - k_special (c0 may be None), rotated by every
        k of ks (odd, at most 16) in one call: for each m the key switch of c1 against keys[m] = [dnum, 2, nm, n], + c0, then the
        NTT-form automorphism by ks[m] -- the permutation last, so the mod-up of c1 is shared.  keys[m] switches from s to
        sigma_(k^-1)(s): a standard Galois key for k becomes it by e.automorphism(key.view(-1, nm, n), kinv, ntt=True).  Returns a
        list of (out0, out1), each [batch, L, n]; `outs` = such a list, else all are views of one new tensor.  plan "sequence" /
        "hoisted" forces a plan.  The first call for a (k_special, alpha), or a larger batch or count, allocates: make it
        before a graph capture.
        level=l (1 to L): c0, c1 and the results are [batch, l, n], a ciphertext below the top level, and every keys[m] is still the
        ONE top-level Galois key (or its first ceil(l / alpha) digits at least), read as key_switch_ntt reads its key at a level."""
        L = self.nmoduli - k_special
        if level is not None:
            self.level_rows(level, k_special)
            L = level
        keys, ks = list(keys), [self._k(k) for k in ks]
        if L <= 0 or c1.numel() % (L * self.degree) or not c1.is_contiguous() or (c0 is not None and (c0.shape != c1.shape or not c0.is_contiguous())):
            raise ValueError("c0 and c1 are contiguous [batch, nm - k_special (or level), n] tensors")
        if len(keys) != len(ks) or not 1 <= len(ks) <= ROTATE_MAX_OUTPUTS:
            raise ValueError("one key per rotation, 1 to 16 rotations")
        batch = c1.numel() // (L * self.degree)
        if not self._level_keys(keys, lambda k: k.numel(), k_special, alpha, level) or any(not k.is_contiguous() for k in keys):
            raise ValueError("every key holds dnum * 2 polynomials of this context")
        if outs is None:
            both = _torch().empty((len(ks), 2, batch, L, self.degree), dtype=self.torch_dtype, device=c1.device)
            outs = [(both[m, 0], both[m, 1]) for m in range(len(ks))]
        p0 = (C.c_void_p * len(ks))(*[o[0].data_ptr() for o in outs])
        p1 = (C.c_void_p * len(ks))(*[o[1].data_ptr() for o in outs])
        pk = (C.c_void_p * len(ks))(*[k.data_ptr() for k in keys])
        kv = (C.c_uint64 * len(ks))(*ks)
        if level is not None:
            self._chk(self.lib.nflhip_rotate_hoisted_level_ntt_dev(self.ctx, p0, p1, _vp(c0), _vp(c1), pk, kv, len(ks), batch, k_special, alpha, level,
                                                                   self._rot_flags(centered, floor, plan), self._stream(stream)))
            return list(outs)
        self._chk(self.lib.nflhip_rotate_hoisted_ntt_dev(self.ctx, p0, p1, _vp(c0), _vp(c1), pk, kv, len(ks), batch, k_special, alpha,
                                                         self._rot_flags(centered, floor, plan), self._stream(stream)))
        return list(outs)

    def h_rotate_hoisted_ntt(self, c0, c1, keys, ks, k_special, alpha, centered=False, floor=False, plan=None, level=None):
        """host-pointer variant: numpy c0 (or None), c1 = [batch, L, n] and keys[m] = [dnum, 2, nm, n] -> a list of (out0, out1);
        level as rotate_hoisted_ntt"""
        c1 = np.ascontiguousarray(c1, dtype=self.np_dtype)
        c0 = None if c0 is None else np.ascontiguousarray(c0, dtype=self.np_dtype)
        keys, ks = [np.ascontiguousarray(k, dtype=self.np_dtype) for k in keys], [self._k(k) for k in ks]
        L = self.nmoduli - k_special
        if level is not None:
            self.level_rows(level, k_special)
            L = level
        if L <= 0 or c1.size % (L * self.degree) or (c0 is not None and c0.shape != c1.shape) or \
                not self._level_keys(keys, lambda k: k.size, k_special, alpha, level):
            raise ValueError("c0, c1 are [batch, nm - k_special (or level), n], every key [dnum, 2, nm, n]")
        if len(keys) != len(ks) or not 1 <= len(ks) <= ROTATE_MAX_OUTPUTS:
            raise ValueError("one key per rotation, 1 to 16 rotations")
        batch = c1.size // (L * self.degree)
        outs = [tuple(np.empty((batch, L, self.degree), dtype=self.np_dtype) for _ in range(2)) for _ in ks]
        p0 = (C.c_void_p * len(ks))(*[o[0].ctypes.data for o in outs])
        p1 = (C.c_void_p * len(ks))(*[o[1].ctypes.data for o in outs])
        pk = (C.c_void_p * len(ks))(*[k.ctypes.data for k in keys])
        kv = (C.c_uint64 * len(ks))(*ks)
        if level is not None:
            self._chk(self.lib.nflhip_rotate_hoisted_level_ntt(self.ctx, p0, p1, _vp(c0), _vp(c1), pk, kv, len(ks), batch, k_special, alpha, level,
                                                               self._rot_flags(centered, floor, plan)))
            return outs
        self._chk(self.lib.nflhip_rotate_hoisted_ntt(self.ctx, p0, p1, _vp(c0), _vp(c1), pk, kv, len(ks), batch, k_special, alpha,
                                                     self._rot_flags(centered, floor, plan)))
        return outs

    # ---- weighted sums of automorphisms and slot linear transforms (include/nflhip.h "weighted sums of automorphisms", "slot
    # linear transforms") ----
    def automorphism_mac(self, ins, weights, ks, addend=None, out=None, rows=None, double_buffer=False, stream=None):
        """addend + sum_t weights[t] * sigma_ks[t](ins[t]) on NTT-form data in ONE launch (at most 16 terms): every ins[t] a contiguous
        [batch, rows, n] tensor over the first `rows` moduli (default: all), every weights[t] a [>= rows, n] tensor shared by the
        batch.  ins may repeat; addend may be `out` itself; out must not overlap an input or a weight.  double_buffer=True stages
        through two buffers instead of one (same words)."""
        ins, weights, ks = list(ins), list(weights), [self._k(k) for k in ks]
        rows = self.nmoduli if rows is None else int(rows)
        if not (len(ins) == len(weights) == len(ks)) or not 1 <= len(ks) <= MAC_MAX_TERMS:
            raise ValueError("one input and one weight per multiplier, 1 to 16 terms")
        if not 1 <= rows <= self.nmoduli or any(x.numel() != ins[0].numel() or x.numel() % (rows * self.degree) or not x.is_contiguous() for x in ins):
            raise ValueError("every input is a contiguous [batch, rows, n] tensor, 1 <= rows <= nm")
        if any(w.numel() < rows * self.degree or not w.is_contiguous() for w in weights):
            raise ValueError("every weight is a contiguous tensor of at least rows * n words")
        batch = ins[0].numel() // (rows * self.degree)
        if out is None:
            out = _torch().empty((batch, rows, self.degree), dtype=self.torch_dtype, device=ins[0].device)
        pi = (C.c_void_p * len(ks))(*[x.data_ptr() for x in ins])
        pw = (C.c_void_p * len(ks))(*[w.data_ptr() for w in weights])
        kv = (C.c_uint64 * len(ks))(*ks)
        self._chk(self.lib.nflhip_automorphism_mac_dev(self.ctx, _vp(out), _vp(addend), pi, pw, kv, len(ks), batch, rows,
                                                       MAC_DOUBLE_BUFFER if double_buffer else 0, self._stream(stream)))
        return out

    def h_automorphism_mac(self, ins, weights, ks, addend=None, rows=None):
        """host-pointer variant: numpy ins[t] = [batch, rows, n], weights[t] = [>= rows, n] -> [batch, rows, n]"""
        ins = [np.ascontiguousarray(x, dtype=self.np_dtype) for x in ins]
        weights, ks = [np.ascontiguousarray(w, dtype=self.np_dtype) for w in weights], [self._k(k) for k in ks]
        rows = self.nmoduli if rows is None else int(rows)
        if not (len(ins) == len(weights) == len(ks)) or not 1 <= len(ks) <= MAC_MAX_TERMS:
            raise ValueError("one input and one weight per multiplier, 1 to 16 terms")
        if not 1 <= rows <= self.nmoduli or any(x.size != ins[0].size or x.size % (rows * self.degree) for x in ins) or \
                any(w.size < rows * self.degree for w in weights):
            raise ValueError("every input is [batch, rows, n], every weight [>= rows, n]")
        batch = ins[0].size // (rows * self.degree)
        addend = None if addend is None else np.ascontiguousarray(addend, dtype=self.np_dtype)
        out = np.empty((batch, rows, self.degree), dtype=self.np_dtype)
        pi = (C.c_void_p * len(ks))(*[x.ctypes.data for x in ins])
        pw = (C.c_void_p * len(ks))(*[w.ctypes.data for w in weights])
        kv = (C.c_uint64 * len(ks))(*ks)
        self._chk(self.lib.nflhip_automorphism_mac(self.ctx, _vp(out), _vp(addend), pi, pw, kv, len(ks), batch, rows, 0))
        return out

    _LT_PLAN = {None: 0, "sequence": LINTRANS_SEQUENCE, "hoisted": LINTRANS_HOISTED}

    def _lt_flags(self, centered, floor, plan):
        return (LINTRANS_CENTERED if centered else 0) | (LINTRANS_FLOOR if floor else 0) | self._LT_PLAN[plan]

    def linear_transform_ntt(self, c0, c1, keys, weights, ks, k_special, alpha, centered=False, floor=False, out=None, plan=None, stream=None,
                             level=None):
        """sum_m weights[m] * sigma_ks[m](ciphertext) in one call with ONE mod-down: (c0, c1) NTT-form [batch, L, n] batches with
        L = nm - k_special (c0 may be None); keys[m] = [dnum, 2, nm, n] by the convention of rotate_hoisted_ntt, or None for the
        unrotated diagonal (ks[m] = 1, no key switch); weights[m] = [nm, n], the diagonal in NTT form over all nm moduli (at most
        16 terms).  The key-switch sums are weighted and added on all nm rows before the mod-down, so the words differ from a
        weighted sum of rotate_hoisted_ntt results by that one rounding.  Returns (out0, out1), each [batch, L, n]; `out` = a
        pair of such tensors, else both are views of one new [2, batch, L, n] tensor.  plan "sequence" / "hoisted" forces a
        plan.  The first call for a (k_special, alpha), or a larger batch or count, allocates: make it before a graph capture.
        level=l (1 to L): c0, c1 and the results are [batch, l, n]; every keys[m] is still the ONE top-level Galois key (or its first
        ceil(l / alpha) digits at least) and every weights[m] the ONE top-level diagonal [nm, n], of which the rows [l, L) are not
        read: a diagonal encoded once serves every level, as a key does."""
        L = self.nmoduli - k_special
        if level is not None:
            self.level_rows(level, k_special)
            L = level
        keys, weights, ks = list(keys), list(weights), [self._k(k) for k in ks]
        if L <= 0 or c1.numel() % (L * self.degree) or not c1.is_contiguous() or (c0 is not None and (c0.shape != c1.shape or not c0.is_contiguous())):
            raise ValueError("c0 and c1 are contiguous [batch, nm - k_special (or level), n] tensors")
        if not (len(keys) == len(weights) == len(ks)) or not 1 <= len(ks) <= LINTRANS_MAX_TERMS:
            raise ValueError("one key (or None) and one weight per term, 1 to 16 terms")
        batch = c1.numel() // (L * self.degree)
        if not self._level_keys(keys, lambda k: k.numel(), k_special, alpha, level) or any(k is not None and not k.is_contiguous() for k in keys):
            raise ValueError("every key holds dnum * 2 polynomials of this context")
        if any(w.numel() != self.words_per_poly or not w.is_contiguous() for w in weights):
            raise ValueError("every weight is one polynomial of this context")
        if out is None:
            both = _torch().empty((2, batch, L, self.degree), dtype=self.torch_dtype, device=c1.device)
            out = (both[0], both[1])
        pk = (C.c_void_p * len(ks))(*[None if k is None else k.data_ptr() for k in keys])
        pw = (C.c_void_p * len(ks))(*[w.data_ptr() for w in weights])
        kv = (C.c_uint64 * len(ks))(*ks)
        if level is not None:
            self._chk(self.lib.nflhip_lintrans_level_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(c0), _vp(c1), pk, pw, kv, len(ks), batch, k_special,
                                                             alpha, level, self._lt_flags(centered, floor, plan), self._stream(stream)))
            return out
        self._chk(self.lib.nflhip_lintrans_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(c0), _vp(c1), pk, pw, kv, len(ks), batch, k_special,
                                                   alpha, self._lt_flags(centered, floor, plan), self._stream(stream)))
        return out

    def h_linear_transform_ntt(self, c0, c1, keys, weights, ks, k_special, alpha, centered=False, floor=False, plan=None, level=None):
        """host-pointer variant: numpy c0 (or None), c1 = [batch, L, n], keys[m] = [dnum, 2, nm, n] or None, weights[m] = [nm, n]
        -> (out0, out1); level as linear_transform_ntt"""
        c1 = np.ascontiguousarray(c1, dtype=self.np_dtype)
        c0 = None if c0 is None else np.ascontiguousarray(c0, dtype=self.np_dtype)
        keys = [None if k is None else np.ascontiguousarray(k, dtype=self.np_dtype) for k in keys]
        weights, ks = [np.ascontiguousarray(w, dtype=self.np_dtype) for w in weights], [self._k(k) for k in ks]
        L = self.nmoduli - k_special
        if level is not None:
            self.level_rows(level, k_special)
            L = level
        if L <= 0 or c1.size % (L * self.degree) or (c0 is not None and c0.shape != c1.shape) or \
                not self._level_keys(keys, lambda k: k.size, k_special, alpha, level) or any(w.size != self.words_per_poly for w in weights):
            raise ValueError("c0, c1 are [batch, nm - k_special (or level), n], every key [dnum, 2, nm, n] or None, every weight [nm, n]")
        if not (len(keys) == len(weights) == len(ks)) or not 1 <= len(ks) <= LINTRANS_MAX_TERMS:
            raise ValueError("one key (or None) and one weight per term, 1 to 16 terms")
        batch = c1.size // (L * self.degree)
        out0, out1 = (np.empty((batch, L, self.degree), dtype=self.np_dtype) for _ in range(2))
        pk = (C.c_void_p * len(ks))(*[None if k is None else k.ctypes.data for k in keys])
        pw = (C.c_void_p * len(ks))(*[w.ctypes.data for w in weights])
        kv = (C.c_uint64 * len(ks))(*ks)
        if level is not None:
            self._chk(self.lib.nflhip_lintrans_level_ntt(self.ctx, _vp(out0), _vp(out1), _vp(c0), _vp(c1), pk, pw, kv, len(ks), batch, k_special, alpha,
                                                         level, self._lt_flags(centered, floor, plan)))
            return out0, out1
        self._chk(self.lib.nflhip_lintrans_ntt(self.ctx, _vp(out0), _vp(out1), _vp(c0), _vp(c1), pk, pw, kv, len(ks), batch, k_special, alpha,
                                               self._lt_flags(centered, floor, plan)))
        return out0, out1

    # ---- several-output weighted sums and BSGS slot linear transforms (include/nflhip.h "weighted sums of automorphisms into several
    # outputs", "BSGS slot linear transforms") ----
    def _mac_multi_args(self, ins, weights, ks, addends, rows, size, contiguous):
        ins, ks = list(ins), [self._k(k) for k in ks]
        weights = [list(w) for w in weights]
        rows = self.nmoduli if rows is None else int(rows)
        if len(ins) != len(ks) or not 1 <= len(ks) <= MAC_MAX_TERMS or not 1 <= len(weights) <= MAC_MULTI_MAX_OUTPUTS or \
                any(len(w) != len(ks) for w in weights):
            raise ValueError("one input per multiplier (1 to 16 terms), one list of weights (or None) per output (1 to 16 outputs)")
        if not 1 <= rows <= self.nmoduli or any(size(x) != size(ins[0]) or size(x) % (rows * self.degree) or not contiguous(x) for x in ins):
            raise ValueError("every input is a contiguous [batch, rows, n] tensor, 1 <= rows <= nm")
        if any(w is not None and (size(w) < rows * self.degree or not contiguous(w)) for ws in weights for w in ws):
            raise ValueError("every weight is None or a contiguous tensor of at least rows * n words")
        addends = [None] * len(weights) if addends is None else list(addends)
        if len(addends) != len(weights):
            raise ValueError("one addend (or None) per output")
        return ins, weights, ks, addends, rows, size(ins[0]) // (rows * self.degree)

    def automorphism_mac_multi(self, ins, weights, ks, addends=None, outs=None, rows=None, stream=None):
        """[addends[o] + sum_t weights[o][t] * sigma_ks[t](ins[t]) for o] on NTT-form data: automorphism_mac for up to 16 outputs that
        share ins and ks, with every term's source staged and permuted once for the outputs of a launch.  weights[o][t] = [>= rows, n]
        or None (the zero weight); addends[o] = None or outs[o] itself; no output may overlap an input, a weight or another output.
        Returns the list of outputs, each [batch, rows, n]."""
        ins, weights, ks, addends, rows, batch = self._mac_multi_args(ins, weights, ks, addends, rows, lambda x: x.numel(), lambda x: x.is_contiguous())
        no = len(weights)
        if outs is None:
            if any(a is not None for a in addends):
                raise ValueError("an addend is its output: pass outs")
            block = _torch().empty((no, batch, rows, self.degree), dtype=self.torch_dtype, device=ins[0].device)
            outs = [block[o] for o in range(no)]
        outs = list(outs)
        if len(outs) != no:
            raise ValueError("one output per list of weights")
        po = (C.c_void_p * no)(*[o.data_ptr() for o in outs])
        pa = (C.c_void_p * no)(*[None if a is None else a.data_ptr() for a in addends])
        pi = (C.c_void_p * len(ks))(*[x.data_ptr() for x in ins])
        pw = (C.c_void_p * (no * len(ks)))(*[None if w is None else w.data_ptr() for ws in weights for w in ws])
        kv = (C.c_uint64 * len(ks))(*ks)
        self._chk(self.lib.nflhip_automorphism_mac_multi_dev(self.ctx, po, pa, pi, pw, kv, no, len(ks), batch, rows, 0, self._stream(stream)))
        return outs

    def h_automorphism_mac_multi(self, ins, weights, ks, addends=None, rows=None):
        """host-pointer variant: numpy ins[t] = [batch, rows, n], weights[o][t] = [>= rows, n] or None, addends[o] = [batch, rows, n] or
        None -> list of [batch, rows, n]"""
        ins = [np.ascontiguousarray(x, dtype=self.np_dtype) for x in ins]
        weights = [[None if w is None else np.ascontiguousarray(w, dtype=self.np_dtype) for w in ws] for ws in weights]
        ins, weights, ks, addends, rows, batch = self._mac_multi_args(ins, weights, ks, addends, rows, lambda x: x.size, lambda x: True)
        no = len(weights)
        outs = [np.empty((batch, rows, self.degree), dtype=self.np_dtype) if a is None else np.array(a, dtype=self.np_dtype).reshape(batch, rows, self.degree)
                for a in addends]
        po = (C.c_void_p * no)(*[o.ctypes.data for o in outs])
        pa = (C.c_void_p * no)(*[None if a is None else o.ctypes.data for a, o in zip(addends, outs)])
        pi = (C.c_void_p * len(ks))(*[x.ctypes.data for x in ins])
        pw = (C.c_void_p * (no * len(ks)))(*[None if w is None else w.ctypes.data for ws in weights for w in ws])
        kv = (C.c_uint64 * len(ks))(*ks)
        self._chk(self.lib.nflhip_automorphism_mac_multi(self.ctx, po, pa, pi, pw, kv, no, len(ks), batch, rows, 0))
        return outs

    _BSGS_PLAN = {None: 0, "sequence": BSGS_SEQUENCE, "hoisted": BSGS_HOISTED}

    def _bsgs_args(self, c0, c1, baby_keys, baby_ks, giant_keys, giant_ks, weights, k_special, alpha, level, size, contiguous):
        L = self.nmoduli - k_special
        lv = L if level is None else int(level)
        self.level_rows(lv, k_special)
        bkeys, gkeys = list(baby_keys), list(giant_keys)
        bks, gks = [self._k(k) for k in baby_ks], [self._k(k) for k in giant_ks]
        weights = [list(w) for w in weights]
        if len(bkeys) != len(bks) or len(gkeys) != len(gks) or not 1 <= len(bks) <= BSGS_MAX_BABY or not 1 <= len(gks) <= BSGS_MAX_GIANT:
            raise ValueError("one key (or None) per step, 1 to 16 baby steps and 1 to 16 giant steps")
        if len(weights) != len(gks) or any(len(w) != len(bks) for w in weights):
            raise ValueError("weights is a list of n2 lists of n1 tensors or None")
        if size(c1) % (lv * self.degree) or not contiguous(c1) or (c0 is not None and (c0.shape != c1.shape or not contiguous(c0))):
            raise ValueError("c0 and c1 are contiguous [batch, level, n] tensors")
        if not self._level_keys(bkeys + gkeys, size, k_special, alpha, level) or \
                any(k is not None and not contiguous(k) for k in bkeys + gkeys):
            raise ValueError("every key holds dnum * 2 polynomials of this context")
        if any(w is not None and (size(w) != self.words_per_poly or not contiguous(w)) for ws in weights for w in ws):
            raise ValueError("every weight is None or one polynomial of this context")
        return bkeys, bks, gkeys, gks, weights, lv, size(c1) // (lv * self.degree)

    def bsgs_linear_transform_ntt(self, c0, c1, baby_keys, baby_ks, giant_keys, giant_ks, weights, k_special, alpha, centered=False, floor=False,
                                  out=None, plan=None, stream=None, level=None):
        """sum_j sigma_giant_ks[j]( sum_i weights[j][i] * sigma_baby_ks[i](ciphertext) ) in one call with ONE mod-down of two polynomials:
        a matrix-vector product by n1 n2 diagonals with n1 + n2 Galois keys.  (c0, c1) NTT-form [batch, l, n] batches, l = level or
        nm - k_special (c0 may be None); baby_keys[i] / giant_keys[j] = the top-level Galois key [dnum, 2, nm, n] by the convention of
        rotate_hoisted_ntt, or None for the unrotated step (k = 1); weights[j][i] = the top-level diagonal [nm, n] in NTT form,
        pre-rotated by sigma_giant_ks[j]^-1, or None for the zero diagonal (every j has one at least).  At most 16 baby and 16 giant
        steps.  Returns (out0, out1), each [batch, l, n]; `out` = a pair of such tensors, else both are views of one new
        [2, batch, l, n] tensor.  plan "sequence" / "hoisted" forces a plan.  The first call for a (k_special, alpha, level, plan), or
        for larger sizes, allocates: make it before a graph capture."""
        bkeys, bks, gkeys, gks, weights, lv, batch = self._bsgs_args(c0, c1, baby_keys, baby_ks, giant_keys, giant_ks, weights, k_special, alpha, level,
                                                                     lambda x: x.numel(), lambda x: x.is_contiguous())
        if out is None:
            both = _torch().empty((2, batch, lv, self.degree), dtype=self.torch_dtype, device=c1.device)
            out = (both[0], both[1])
        pb = (C.c_void_p * len(bks))(*[None if k is None else k.data_ptr() for k in bkeys])
        pg = (C.c_void_p * len(gks))(*[None if k is None else k.data_ptr() for k in gkeys])
        pw = (C.c_void_p * (len(bks) * len(gks)))(*[None if w is None else w.data_ptr() for ws in weights for w in ws])
        kb, kg = (C.c_uint64 * len(bks))(*bks), (C.c_uint64 * len(gks))(*gks)
        flags = (BSGS_CENTERED if centered else 0) | (BSGS_FLOOR if floor else 0) | self._BSGS_PLAN[plan]
        self._chk(self.lib.nflhip_bsgs_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(c0), _vp(c1), pb, kb, len(bks), pg, kg, len(gks), pw, batch,
                                               k_special, alpha, lv, flags, self._stream(stream)))
        return out

    def h_bsgs_linear_transform_ntt(self, c0, c1, baby_keys, baby_ks, giant_keys, giant_ks, weights, k_special, alpha, centered=False, floor=False,
                                    plan=None, level=None):
        """host-pointer variant: numpy operands as bsgs_linear_transform_ntt -> (out0, out1)"""
        def arr(x):
            return None if x is None else np.ascontiguousarray(x, dtype=self.np_dtype)
        c0, c1 = arr(c0), arr(c1)
        bkeys, bks, gkeys, gks, weights, lv, batch = self._bsgs_args(c0, c1, [arr(k) for k in baby_keys], baby_ks, [arr(k) for k in giant_keys], giant_ks,
                                                                     [[arr(w) for w in ws] for ws in weights], k_special, alpha, level,
                                                                     lambda x: x.size, lambda x: True)
        out0, out1 = (np.empty((batch, lv, self.degree), dtype=self.np_dtype) for _ in range(2))
        pb = (C.c_void_p * len(bks))(*[None if k is None else k.ctypes.data for k in bkeys])
        pg = (C.c_void_p * len(gks))(*[None if k is None else k.ctypes.data for k in gkeys])
        pw = (C.c_void_p * (len(bks) * len(gks)))(*[None if w is None else w.ctypes.data for ws in weights for w in ws])
        kb, kg = (C.c_uint64 * len(bks))(*bks), (C.c_uint64 * len(gks))(*gks)
        flags = (BSGS_CENTERED if centered else 0) | (BSGS_FLOOR if floor else 0) | self._BSGS_PLAN[plan]
        self._chk(self.lib.nflhip_bsgs_ntt(self.ctx, _vp(out0), _vp(out1), _vp(c0), _vp(c1), pb, kb, len(bks), pg, kg, len(gks), pw, batch, k_special, alpha,
                                           lv, flags))
        return out0, out1

    # ---- ciphertext multiplication (include/nflhip.h "ciphertext multiplication") ----
    _MR_PLAN = {None: 0, "sequence": MULRELIN_SEQUENCE, "merged": MULRELIN_MERGED, "fused": MULRELIN_FUSED}

    def _mr_flags(self, rescale, centered, floor, plan):
        return (MULRELIN_RESCALE if rescale else 0) | (MULRELIN_CENTERED if centered else 0) | (MULRELIN_FLOOR if floor else 0) | self._MR_PLAN[plan]

    def _tensor_rows(self, a0, a1, b0, b1, rows, size, contiguous):
        rows = self.nmoduli if rows is None else rows
        if (b0 is None) != (b1 is None):
            raise ValueError("b0 and b1 are both given, or both None for the square")
        ops = [x for x in (a0, a1, b0, b1) if x is not None]
        if not 1 <= rows <= self.nmoduli or size(a0) % (rows * self.degree) or any(size(x) != size(a0) or not contiguous(x) for x in ops):
            raise ValueError("a0, a1, b0, b1 are contiguous [batch, rows, n] blocks of one size")
        return rows, size(a0) // (rows * self.degree)

    def tensor_ntt(self, a0, a1, b0=None, b1=None, rows=None, outs=None, stream=None):
        """the tensor product of the ciphertexts (a0, a1) and (b0, b1), each component a [batch, rows, n] block over the first `rows`
        moduli (default: all): (a0 b0, a0 b1 + a1 b0, a1 b1) row by row, one launch.  b0 = b1 = None: the square, (a0^2, 2 a0 a1,
        a1^2).  `outs` = three such tensors (any may be one of the inputs), else views of one new [3, batch, rows, n] tensor."""
        rows, batch = self._tensor_rows(a0, a1, b0, b1, rows, lambda x: x.numel(), lambda x: x.is_contiguous())
        if outs is None:
            o = _torch().empty((3, batch, rows, self.degree), dtype=self.torch_dtype, device=a0.device)
            outs = (o[0], o[1], o[2])
        elif len(outs) != 3 or any(o.numel() != a0.numel() or not o.is_contiguous() for o in outs):
            raise ValueError("outs are three contiguous [batch, rows, n] tensors")
        self._chk(self.lib.nflhip_tensor_ntt_dev(self.ctx, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), batch, rows,
                                                 0, self._stream(stream)))
        return outs

    def h_tensor_ntt(self, a0, a1, b0=None, b1=None, rows=None):
        """host-pointer variant: numpy blocks [batch, rows, n] -> (out0, out1, out2)"""
        a0, a1, b0, b1 = (None if x is None else np.ascontiguousarray(x, dtype=self.np_dtype) for x in (a0, a1, b0, b1))
        rows, batch = self._tensor_rows(a0, a1, b0, b1, rows, lambda x: x.size, lambda x: True)
        outs = tuple(np.empty((batch, rows, self.degree), dtype=self.np_dtype) for _ in range(3))
        self._chk(self.lib.nflhip_tensor_ntt(self.ctx, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), batch, rows, 0))
        return outs

    # ---- BFV multiplication (include/nflhip.h "BFV multiplication") ----
    _SR_PLAN = {None: 0, "two_pass": SCALE_ROUND_TWO_PASS}

    def _sr_flags(self, floor, keep, plan):
        return (SCALE_ROUND_FLOOR if floor else 0) | (SCALE_ROUND_KEEP if keep else 0) | self._SR_PLAN[plan]

    def scale_round(self, a, ks, t, floor=False, keep=False, ntt=False, out=None, plan=None, stream=None):
        """round(t X / Q) of the batch a = [batch, nm, n], Q the product of the first ks moduli, carried back onto those rows: a new
        [batch, ks, n] tensor in the layout of Engine(limb_bits, degree, ks) (or `out`, which must not overlap a).  keep=True stops
        at the words Y on the other rows: [batch, nm - ks, n].  floor=True: the fast first conversion, floor(t X / Q) - u.  ntt=True:
        NTT form in and out.  plan="two_pass" forces the two-pass plan.  The first call for a (ks, t) uploads its tables (and the
        two-pass plan and the NTT form allocate scratch): make it before a graph capture."""
        batch = self._batch(a)
        if out is None:
            rows = self.nmoduli - ks if keep else ks
            out = _torch().empty((batch, max(rows, 0), self.degree), dtype=self.torch_dtype, device=a.device)
        fn = self.lib.nflhip_scale_round_ntt_dev if ntt else self.lib.nflhip_scale_round_dev
        self._chk(fn(self.ctx, _vp(out), _vp(a), batch, ks, t, self._sr_flags(floor, keep, plan), self._stream(stream)))
        return out

    def h_scale_round(self, a, ks, t, floor=False, keep=False, ntt=False, plan=None):
        """host-pointer variant: a numpy [batch, nm, n] batch -> [batch, ks, n] ([batch, nm - ks, n] with keep)"""
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        batch = self._hb(a)
        out = np.empty((batch, max(self.nmoduli - ks if keep else ks, 0), self.degree), dtype=self.np_dtype)
        fn = self.lib.nflhip_scale_round_ntt if ntt else self.lib.nflhip_scale_round
        self._chk(fn(self.ctx, _vp(out), _vp(a), batch, ks, t, self._sr_flags(floor, keep, plan)))
        return out

    def bfv_tensor_ntt(self, a0, a1, b0, b1, L, t, floor=False, outs=None, plan=None, stream=None):
        """the scale-invariant tensor product of the BFV ciphertexts (a0, a1) and (b0, b1), NTT-form [batch, L, n] blocks over the first
        L moduli of this context (the other nm - L are the extension B): base extension, tensor product on nm rows, round(t . / Q)
        back onto the L rows.  b0 = b1 = None: the square.  `outs` = three [batch, L, n] tensors (any may be one of the inputs), else
        views of one new [3, batch, L, n] tensor.  The first call for an (L, t), or a larger batch, allocates."""
        rows, batch = self._tensor_rows(a0, a1, b0, b1, L, lambda x: x.numel(), lambda x: x.is_contiguous())
        if outs is None:
            o = _torch().empty((3, batch, rows, self.degree), dtype=self.torch_dtype, device=a0.device)
            outs = (o[0], o[1], o[2])
        elif len(outs) != 3 or any(o.numel() != a0.numel() or not o.is_contiguous() for o in outs):
            raise ValueError("outs are three contiguous [batch, L, n] tensors")
        self._chk(self.lib.nflhip_bfv_tensor_ntt_dev(self.ctx, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), batch, rows,
                                                     t, self._sr_flags(floor, False, plan), self._stream(stream)))
        return outs

    def h_bfv_tensor_ntt(self, a0, a1, b0, b1, L, t, floor=False, plan=None):
        """host-pointer variant: numpy blocks [batch, L, n] -> (out0, out1, out2)"""
        a0, a1, b0, b1 = (None if x is None else np.ascontiguousarray(x, dtype=self.np_dtype) for x in (a0, a1, b0, b1))
        rows, batch = self._tensor_rows(a0, a1, b0, b1, L, lambda x: x.size, lambda x: True)
        outs = tuple(np.empty((batch, rows, self.degree), dtype=self.np_dtype) for _ in range(3))
        self._chk(self.lib.nflhip_bfv_tensor_ntt(self.ctx, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), batch, rows, t,
                                                 self._sr_flags(floor, False, plan)))
        return outs

    def bfv_mul_relin_ntt(self, ks_engine, a0, a1, b0, b1, key, L, t, K, alpha, floor=False, plan=None, stream=None):
        """the product of two BFV ciphertexts with relinearisation: bfv_tensor_ntt on this context (the first L + kb moduli), the key
        switch of its third component by ks_engine -- the engine over the first L + K moduli, key = [dnum, 2, L + K, n] from s^2 to s
        as key_switch_ntt takes it -- and the two sums.  A thin composition, no entry of its own.  Returns (out0, out1), [batch, L, n]."""
        if ks_engine.nmoduli != L + K or ks_engine.limb_bits != self.limb_bits or ks_engine.degree != self.degree:
            raise ValueError("ks_engine is the engine over the first L + K moduli")
        d0, d1, d2 = self.bfv_tensor_ntt(a0, a1, b0, b1, L, t, floor=floor, plan=plan, stream=stream)
        k0, k1 = ks_engine.key_switch_ntt(d2, key, K, alpha, stream=stream)
        kept = getattr(self, "_bfv_kept", None)
        if kept is None or kept.nmoduli != L:
            kept = self._bfv_kept = Engine(self.limb_bits, self.degree, L, device=self.device)
        return kept.pointwise(OP_ADD, d0, k0, out=d0, stream=stream), kept.pointwise(OP_ADD, d1, k1, out=d1, stream=stream)

    def mul_relin_ntt(self, a0, a1, b0, b1, key, k_special, alpha, rescale=False, centered=False, floor=False, out=None, plan=None, stream=None,
                      level=None):
        """the product of the ciphertexts (a0, a1) and (b0, b1) with relinearisation, one call: NTT-form [batch, L, n] batches with
        L = nm - k_special (b0 = b1 = None: the square), key = [dnum, 2, nm, n] as key_switch_ntt takes it, from s^2 to s.  The tensor
        product's first two components go into the key-switch sums of the third before the ONE mod-down.  rescale=True divides by
        the last kept modulus in the same rounding: the results are [batch, L - 1, n].  Returns (out0, out1); `out` = a pair of
        such tensors (each may be one of the inputs), else both are views of one new [2, batch, L or L - 1, n] tensor.  plan
        "sequence" / "merged" / "fused" forces a plan.  The first call for a (k_special, alpha), or a larger batch, allocates: make it before
        a graph capture.
        level=l (1 to L; 2 at least with rescale): the operands are [batch, l, n], the results [batch, l or l - 1, n], and the key is
        still the ONE top-level key, read as key_switch_ntt reads it at a level -- so the result of a rescaling product can be
        multiplied again."""
        L = self.nmoduli - k_special
        if L <= 0:
            raise ValueError("k_special is 1 to nm - 1")
        if level is not None:
            self.level_rows(level, k_special)
            if rescale and level < 2:
                raise ValueError("the rescale needs level >= 2")
            L = level
        _, batch = self._tensor_rows(a0, a1, b0, b1, L, lambda x: x.numel(), lambda x: x.is_contiguous())
        if not key.is_contiguous():
            raise ValueError("key holds dnum * 2 polynomials of this context")
        if level is not None:
            self._level_key(key.numel(), k_special, alpha, level)
        elif key.numel() != 2 * self.keyswitch_digits(k_special, alpha) * self.words_per_poly:
            raise ValueError("key holds dnum * 2 polynomials of this context")
        if out is None:
            both = _torch().empty((2, batch, L - 1 if rescale else L, self.degree), dtype=self.torch_dtype, device=a0.device)
            out = (both[0], both[1])
        elif len(out) != 2 or any(o.numel() != batch * (L - 1 if rescale else L) * self.degree or not o.is_contiguous() for o in out):
            raise ValueError("out is a pair of contiguous [batch, L, n] tensors ([batch, L - 1, n] with rescale)")
        if level is not None:
            self._chk(self.lib.nflhip_mulrelin_level_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), _vp(key), batch,
                                                             k_special, alpha, level, self._mr_flags(rescale, centered, floor, plan),
                                                             self._stream(stream)))
            return out
        self._chk(self.lib.nflhip_mulrelin_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), _vp(key), batch, k_special,
                                                   alpha, self._mr_flags(rescale, centered, floor, plan), self._stream(stream)))
        return out

    def h_mul_relin_ntt(self, a0, a1, b0, b1, key, k_special, alpha, rescale=False, centered=False, floor=False, plan=None, level=None):
        """host-pointer variant: numpy a0, a1, b0, b1 = [batch, L, n] (b0 = b1 = None: the square), key = [dnum, 2, nm, n] -> (out0, out1);
        level as mul_relin_ntt"""
        a0, a1, b0, b1 = (None if x is None else np.ascontiguousarray(x, dtype=self.np_dtype) for x in (a0, a1, b0, b1))
        key = np.ascontiguousarray(key, dtype=self.np_dtype)
        if level is not None:
            self.level_rows(level, k_special)
            if rescale and level < 2:
                raise ValueError("the rescale needs level >= 2")
            self._level_key(key.size, k_special, alpha, level)
            _, batch = self._tensor_rows(a0, a1, b0, b1, level, lambda x: x.size, lambda x: True)
            out0, out1 = (np.empty((batch, level - 1 if rescale else level, self.degree), dtype=self.np_dtype) for _ in range(2))
            self._chk(self.lib.nflhip_mulrelin_level_ntt(self.ctx, _vp(out0), _vp(out1), _vp(a0), _vp(a1), _vp(b0), _vp(b1), _vp(key), batch, k_special,
                                                         alpha, level, self._mr_flags(rescale, centered, floor, plan)))
            return out0, out1
        L = self.nmoduli - k_special
        if L <= 0 or key.size != 2 * self.keyswitch_digits(k_special, alpha) * self.words_per_poly:
            raise ValueError("k_special is 1 to nm - 1, key [dnum, 2, nm, n]")
        _, batch = self._tensor_rows(a0, a1, b0, b1, L, lambda x: x.size, lambda x: True)
        out0, out1 = (np.empty((batch, L - 1 if rescale else L, self.degree), dtype=self.np_dtype) for _ in range(2))
        self._chk(self.lib.nflhip_mulrelin_ntt(self.ctx, _vp(out0), _vp(out1), _vp(a0), _vp(a1), _vp(b0), _vp(b1), _vp(key), batch, k_special, alpha,
                                               self._mr_flags(rescale, centered, floor, plan)))
        return out0, out1

    # ---- sums of ciphertext products (include/nflhip.h "sums of ciphertext products") ----
    @staticmethod
    def _dot_operand(x, strides):
        return _lib.DotOperand(x if isinstance(x, int) else x.data_ptr(), strides[0], strides[1])

    def _dot_operands(self, a0, a1, b0, b1):
        """four (tensor_or_address, (group_stride, term_stride)) pairs -> the ctypes operands (b0 = b1 = None: the squares)"""
        if (b0 is None) != (b1 is None):
            raise ValueError("b0 and b1 are both given, or both None for the squares")
        ops = [None if x is None else self._dot_operand(*x) for x in (a0, a1, b0, b1)]
        return ops, [None if o is None else C.byref(o) for o in ops]

    def _dot_blocks(self, a0, a1, b0, b1, terms, rows, b_shared, size):
        """dense blocks [groups * terms, rows, n] (b: [terms, rows, n] with b_shared) -> groups"""
        if (b0 is None) != (b1 is None):
            raise ValueError("b0 and b1 are both given, or both None for the squares")
        poly = rows * self.degree
        if terms <= 0 or size(a0) % (terms * poly) or size(a1) != size(a0):
            raise ValueError("a0 and a1 hold groups * terms polynomials of `rows` rows each")
        groups = size(a0) // (terms * poly)
        if b0 is not None and any(size(x) != (terms * poly if b_shared else size(a0)) for x in (b0, b1)):
            raise ValueError("b0 and b1 hold groups * terms polynomials, or terms with b_shared")
        return groups

    def tensor_dot_strided(self, a0, a1, b0, b1, groups, terms, rows=None, outs=None, stream=None):
        """tensor_dot_ntt on operands anywhere: each of a0, a1, b0, b1 is (tensor_or_address, (group_stride, term_stride)) as
        dot_strided takes them, the strides in polynomials of `rows` rows (b0 = b1 = None: the squares); the outputs must not
        overlap the operands"""
        rows = self.nmoduli if rows is None else rows
        keep, refs = self._dot_operands(a0, a1, b0, b1)
        if outs is None:
            o = _torch().empty((3, groups, max(rows, 0), self.degree), dtype=self.torch_dtype, device="cuda:%d" % self.device)
            outs = (o[0], o[1], o[2])
        self._chk(self.lib.nflhip_tensor_dot_ntt_dev(self.ctx, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), refs[0], refs[1], refs[2], refs[3], groups, terms,
                                                     rows, 0, self._stream(stream)))
        return outs

    def tensor_dot_ntt(self, a0, a1, b0=None, b1=None, terms=1, rows=None, b_shared=False, outs=None, stream=None):
        """the tensor products of `terms` pairs of ciphertexts summed per group, one launch: a0, a1 = [groups * terms, rows, n] blocks
        over the first `rows` moduli (default: all), b0, b1 alike, or [terms, rows, n] shared by every group with b_shared;
        (D0, D1, D2)[g] = sum_j (a0 b0, a0 b1 + a1 b0, a1 b1)(g, j).  b0 = b1 = None: the sums of squares.  `outs` = three
        [groups, rows, n] tensors apart from the operands, else views of one new [3, groups, rows, n] tensor."""
        rows = self.nmoduli if rows is None else rows
        if not 1 <= rows <= self.nmoduli or any(x is not None and not x.is_contiguous() for x in (a0, a1, b0, b1)):
            raise ValueError("rows is 1 to nm; the operands are contiguous")
        groups = self._dot_blocks(a0, a1, b0, b1, terms, rows, b_shared, lambda x: x.numel())
        sb = (0 if b_shared else terms, 1)
        return self.tensor_dot_strided((a0, (terms, 1)), (a1, (terms, 1)), None if b0 is None else (b0, sb), None if b1 is None else (b1, sb),
                                       groups, terms, rows, outs, stream)

    def h_tensor_dot_ntt(self, a0, a1, b0=None, b1=None, terms=1, rows=None, b_shared=False):
        """host-pointer variant: numpy blocks as tensor_dot_ntt takes them -> (D0, D1, D2), each [groups, rows, n]"""
        a0, a1, b0, b1 = (None if x is None else np.ascontiguousarray(x, dtype=self.np_dtype) for x in (a0, a1, b0, b1))
        rows = self.nmoduli if rows is None else rows
        if not 1 <= rows <= self.nmoduli:
            raise ValueError("rows is 1 to nm")
        groups = self._dot_blocks(a0, a1, b0, b1, terms, rows, b_shared, lambda x: x.size)
        outs = tuple(np.empty((groups, rows, self.degree), dtype=self.np_dtype) for _ in range(3))
        self._chk(self.lib.nflhip_tensor_dot_ntt(self.ctx, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(a0), _vp(a1), _vp(b0), _vp(b1), groups, terms,
                                                 int(bool(b_shared)), rows, 0))
        return outs

    def _mr_dot_level(self, k_special, rescale, level):
        L = self.nmoduli - k_special
        if L <= 0:
            raise ValueError("k_special is 1 to nm - 1")
        level = L if level is None else level
        self.level_rows(level, k_special)
        if rescale and level < 2:
            raise ValueError("the rescale needs level >= 2")
        return level

    def mul_relin_dot_strided(self, a0, a1, b0, b1, groups, terms, key, k_special, alpha, rescale=False, centered=False, floor=False, out=None, plan=None,
                              stream=None, level=None):
        """mul_relin_dot_ntt on operands anywhere: each of a0, a1, b0, b1 is (tensor_or_address, (group_stride, term_stride)), the
        strides in polynomials of `level` rows (b0 = b1 = None: the squares).  An output is apart from an operand's extent or begins
        at its first byte."""
        level = self._mr_dot_level(k_special, rescale, level)
        if not key.is_contiguous():
            raise ValueError("key holds dnum * 2 polynomials of this context")
        self._level_key(key.numel(), k_special, alpha, level)
        keep, refs = self._dot_operands(a0, a1, b0, b1)
        if out is None:
            both = _torch().empty((2, groups, level - 1 if rescale else level, self.degree), dtype=self.torch_dtype, device=key.device)
            out = (both[0], both[1])
        elif len(out) != 2 or any(o.numel() != groups * (level - 1 if rescale else level) * self.degree or not o.is_contiguous() for o in out):
            raise ValueError("out is a pair of contiguous [groups, level, n] tensors ([groups, level - 1, n] with rescale)")
        self._chk(self.lib.nflhip_mulrelin_dot_ntt_dev(self.ctx, _vp(out[0]), _vp(out[1]), refs[0], refs[1], refs[2], refs[3], _vp(key), groups, terms,
                                                       k_special, alpha, level, self._mr_flags(rescale, centered, floor, plan), self._stream(stream)))
        return out

    def mul_relin_dot_ntt(self, a0, a1, b0, b1, terms, key, k_special, alpha, b_shared=False, rescale=False, centered=False, floor=False, out=None,
                          plan=None, stream=None, level=None):
        """sum_j ct_a[g, j] * ct_b[g, j] per group with ONE relinearisation: the tensor products are summed first and the degree-2
        component key-switched once -- one mod-up, one inner product against the key, one mod-down and one key-switch noise term for
        `terms` products.  a0, a1 = NTT-form [groups * terms, l, n] blocks, l = level (default: the top, nm - k_special); b0, b1 alike,
        or [terms, l, n] shared by every group with b_shared; b0 = b1 = None: the sum of squares.  key, rescale, centered, floor and
        level as mul_relin_ntt.  Returns (out0, out1), each [groups, l or l - 1, n]: `out`, else views of one new tensor, adjacent
        so that one mod-down serves both.  plan "sequence" / "merged"; "fused" serves terms == 1 with dense operands only, where
        the call is mul_relin_ntt.  The first call for a (k_special, alpha), or for more groups, allocates."""
        level = self._mr_dot_level(k_special, rescale, level)
        if any(x is not None and not x.is_contiguous() for x in (a0, a1, b0, b1)):
            raise ValueError("the operands are contiguous")
        groups = self._dot_blocks(a0, a1, b0, b1, terms, level, b_shared, lambda x: x.numel())
        sb = (0 if b_shared else terms, 1)
        return self.mul_relin_dot_strided((a0, (terms, 1)), (a1, (terms, 1)), None if b0 is None else (b0, sb), None if b1 is None else (b1, sb),
                                          groups, terms, key, k_special, alpha, rescale, centered, floor, out, plan, stream, level)

    def h_mul_relin_dot_ntt(self, a0, a1, b0, b1, terms, key, k_special, alpha, b_shared=False, rescale=False, centered=False, floor=False, plan=None,
                            level=None):
        """host-pointer variant: numpy blocks as mul_relin_dot_ntt takes them, key = [dnum, 2, nm, n] -> (out0, out1)"""
        a0, a1, b0, b1 = (None if x is None else np.ascontiguousarray(x, dtype=self.np_dtype) for x in (a0, a1, b0, b1))
        key = np.ascontiguousarray(key, dtype=self.np_dtype)
        level = self._mr_dot_level(k_special, rescale, level)
        self._level_key(key.size, k_special, alpha, level)
        groups = self._dot_blocks(a0, a1, b0, b1, terms, level, b_shared, lambda x: x.size)
        out0, out1 = (np.empty((groups, level - 1 if rescale else level, self.degree), dtype=self.np_dtype) for _ in range(2))
        self._chk(self.lib.nflhip_mulrelin_dot_ntt(self.ctx, _vp(out0), _vp(out1), _vp(a0), _vp(a1), _vp(b0), _vp(b1), _vp(key), groups, terms,
                                                   int(bool(b_shared)), k_special, alpha, level, self._mr_flags(rescale, centered, floor, plan)))
        return out0, out1

    def pointwise(self, op, a, b=None, bprime=None, out=None, stream=None):
        out = out if out is not None else _torch().empty_like(a)
        self._chk(self.lib.nflhip_pointwise_dev(self.ctx, op, _vp(out), _vp(a), _vp(b), _vp(bprime), self._batch(a),
                                                self._stream(stream)))
        return out

    def eval(self, program, operands, out=None, stream=None):
        """Fused expression tree: `program` = postfix bytes (k<8 push operand k, 0x10 add, 0x11 sub,
        0x12 mul, 0x13 mul_shoup, 0x14 compute_shoup), one device pass (nflhip_eval_dev)."""
        out = out if out is not None else _torch().empty_like(operands[0])
        ptrs = (C.c_void_p * len(operands))(*[o.data_ptr() for o in operands])
        prog = (C.c_ubyte * len(program))(*program)
        self._chk(self.lib.nflhip_eval_dev(self.ctx, _vp(out), C.cast(ptrs, C.c_void_p), len(operands),
                                           C.cast(prog, C.c_void_p), len(program), self._batch(operands[0]),
                                           self._stream(stream)))
        return out

    def eval_strided(self, program, operands, strides, out, out_stride=1, batch=None, stream=None):
        """nflhip_eval_strided_dev: element i reads operand j at operands[j] + i*strides[j] polynomials (0 = one shared
        polynomial) and writes out + i*out_stride polynomials"""
        if len(strides) != len(operands):
            raise ValueError("one stride per operand")
        if not out.is_contiguous() or not all(o.is_contiguous() for o in operands):
            raise ValueError("operands and result must be contiguous tensors")
        if batch is None:   # the elements the result buffer holds at this stride
            batch = (self._batch(out) + out_stride - 1) // out_stride
        ptrs = (C.c_void_p * len(operands))(*[o.data_ptr() for o in operands])
        sd = (C.c_size_t * len(operands))(*strides)
        prog = (C.c_ubyte * len(program))(*program)
        self._chk(self.lib.nflhip_eval_strided_dev(self.ctx, _vp(out), out_stride, C.cast(ptrs, C.c_void_p),
                                                   C.cast(sd, C.c_void_p), len(operands), C.cast(prog, C.c_void_p),
                                                   len(program), batch, self._stream(stream)))
        return out

    def h_eval(self, program, operands):
        out = np.empty_like(operands[0])
        ptrs = (C.c_void_p * len(operands))(*[o.ctypes.data for o in operands])
        prog = (C.c_ubyte * len(program))(*program)
        self._chk(self.lib.nflhip_eval(self.ctx, _vp(out), C.cast(ptrs, C.c_void_p), len(operands),
                                       C.cast(prog, C.c_void_p), len(program), self._hb(operands[0])))
        return out

    def polymul(self, a, b, out=None, b_is_ntt=False, stream=None):
        out = out if out is not None else _torch().empty_like(a)
        fn = self.lib.nflhip_polymul_ntt_dev if b_is_ntt else self.lib.nflhip_polymul_dev
        self._chk(fn(self.ctx, _vp(out), _vp(a), _vp(b), self._batch(a), self._stream(stream)))
        return out

    # ---- transform-fused pipelines (include/nflhip.h "transform-fused pipelines") ----
    def _operand(self, ten, words_only=False):
        """nflhip_operand of a tensor: [count][nmoduli][degree] limb words, or -- forward inputs -- [count][degree] int8 /
        int16 / int32 (one signed integer per coefficient); count 1 = one polynomial for the whole batch (stride 0)"""
        t = _torch()
        if not ten.is_contiguous():
            raise ValueError("operands must be contiguous tensors")
        # the shape names the format (torch has no unsigned 16 / 32-bit types, so a u16 / u32 ring's words share int16 / int32
        # with the compact formats): limb words are 3-D [count][nmoduli][degree], compact polynomials 2-D [count][degree];
        # anything else is ambiguous and refused
        compact = {t.int8: FMT_I8, t.int16: FMT_I16, t.int32: FMT_I32}.get(ten.dtype)
        if ten.dim() == 3 and ten.dtype == self.torch_dtype and tuple(ten.shape[1:]) == (self.nmoduli, self.degree):
            fmt = FMT_WORDS
        elif ten.dim() == 2 and compact is not None and ten.shape[1] == self.degree and not words_only:
            fmt = compact
        else:
            raise ValueError("operand shape / dtype: limb words are [count][nmoduli][degree] of the ring's word type, compact "
                             "polynomials [count][degree] int8 / int16 / int32")
        per = self.degree if fmt != FMT_WORDS else self.words_per_poly
        count = ten.numel() // per
        return _lib.Operand(ten.data_ptr(), 0 if count == 1 else 1, fmt), count

    def fwd_fma(self, x, k, e, out=None, batch=None, stream=None):
        """out = NTT(x) * k + NTT(e) in one pass (nflhip_fwd_fma_dev)"""
        (ox, nx), (ok, nk), (oe, ne) = self._operand(x), self._operand(k, True), self._operand(e)
        batch = batch if batch is not None else max(nx, nk, ne)
        out = out if out is not None else self.empty(batch)
        self._chk(self.lib.nflhip_fwd_fma_dev(self.ctx, _vp(out), C.byref(ox), C.byref(ok), C.byref(oe), batch, self._stream(stream)))
        return out

    def fwd_fma2(self, x, k0, e0, k1, e1, out0=None, out1=None, batch=None, stream=None):
        """out0 = NTT(x) * k0 + NTT(e0), out1 = NTT(x) * k1 + NTT(e1) in one pass: the LWE demo's encrypt()
        (tests/nfllib_demo_main_op.cpp:26-46) for the whole batch (nflhip_fwd_fma2_dev)"""
        ops = [self._operand(x), self._operand(k0, True), self._operand(e0), self._operand(k1, True), self._operand(e1)]
        batch = batch if batch is not None else max(n for _, n in ops)
        out0 = out0 if out0 is not None else self.empty(batch)
        out1 = out1 if out1 is not None else self.empty(batch)
        self._chk(self.lib.nflhip_fwd_fma2_dev(self.ctx, _vp(out0), _vp(out1), *[C.byref(o) for o, _ in ops], batch, self._stream(stream)))
        return out0, out1

    def fma_inv(self, a, k, b, subtract=False, out=None, batch=None, stream=None):
        """out = INTT(b + a * k) or INTT(b - a * k): the demo's decrypt() (tests/nfllib_demo_main_op.cpp:49-51)"""
        (oa, na), (ok, nk), (ob, nb) = self._operand(a, True), self._operand(k, True), self._operand(b, True)
        batch = batch if batch is not None else max(na, nk, nb)
        out = out if out is not None else self.empty(batch)
        self._chk(self.lib.nflhip_fma_inv_dev(self.ctx, _vp(out), C.byref(oa), C.byref(ok), C.byref(ob), int(bool(subtract)), batch,
                                              self._stream(stream)))
        return out

    def expand_small(self, src, batch=None, out=None, stream=None):
        """compact polynomials (one signed integer per coefficient) -> residue words (nflhip_expand_small_dev)"""
        o, n = self._operand(src)
        batch = batch if batch is not None else n
        out = out if out is not None else self.empty(batch)
        self._chk(self.lib.nflhip_expand_small_dev(self.ctx, _vp(out), C.byref(o), batch, self._stream(stream)))
        return out

    def empty_small(self, batch, fmt=FMT_I8):
        t = _torch()
        return t.empty((batch, self.degree), dtype={FMT_I8: t.int8, FMT_I16: t.int16, FMT_I32: t.int32}[fmt], device="cuda:%d" % self.device)

    def sample_gauss_small(self, d, g, key, stream_id=None, amplifier=1, first_poly=0, stream=None):
        """compact Gaussian polynomials: d[b][i] = sample * amplifier as int8 / int16 / int32 (the tensor's dtype), the same
        samples sample_gauss spreads over the moduli"""
        o, n = self._operand(d)
        self._chk(self.lib.nflhip_sample_gauss_small_dev(self.ctx, _vp(d), o.format, first_poly, n, g, amplifier, self._key(key),
                                                         self._sid(stream_id), self._stream(stream)))
        return d

    def sample_gauss_small_seq(self, d, g, key, first_stream_id, stream_id_stride=1, amplifier=1, stream=None):
        o, n = self._operand(d)
        self._chk(self.lib.nflhip_sample_gauss_small_seq_dev(self.ctx, _vp(d), o.format, n, g, amplifier, self._key(key),
                                                             first_stream_id, stream_id_stride, self._stream(stream)))
        return d

    def sample_gauss_small_multi(self, ds, g, key, stream_ids, stream_id_strides=None, amplifiers=None, stream=None):
        """up to four compact draws of one table in ONE launch (nflhip_sample_gauss_small_multi_dev): draw j fills ds[j] exactly as
        sample_gauss_small_seq(ds[j], g, key, stream_ids[j], stream_id_strides[j], amplifiers[j]) would -- or, without strides, as
        sample_gauss_small(ds[j], g, key, stream_ids[j], amplifiers[j])"""
        cnt = len(ds)
        o, n = self._operand(ds[0])
        amplifiers = list(amplifiers) if amplifiers is not None else [1] * cnt
        ptrs = (C.c_void_p * cnt)(*[d.data_ptr() for d in ds])
        amps = (C.c_uint64 * cnt)(*amplifiers)
        sids = (C.c_uint64 * cnt)(*stream_ids)
        strides = (C.c_uint64 * cnt)(*stream_id_strides) if stream_id_strides is not None else None
        self._chk(self.lib.nflhip_sample_gauss_small_multi_dev(self.ctx, ptrs, cnt, o.format, n, g, amps, self._key(key), sids, strides,
                                                               self._stream(stream)))
        return ds

    def check_range(self, d, stream=None):
        """CHECK_STRICTMOD's assertion over a resident batch: True iff some word is >= its row's modulus"""
        r = C.c_int(0)
        self._chk(self.lib.nflhip_check_range_dev(self.ctx, _vp(d), self._batch(d), C.byref(r), self._stream(stream)))
        return bool(r.value)

    def h_check_range(self, a):
        r = C.c_int(0)
        self._chk(self.lib.nflhip_check_range(self.ctx, _vp(a), self._hb(a), C.byref(r)))
        return bool(r.value)

    def any_eq(self, a, b, stream=None):
        r = C.c_int(0)
        self._chk(self.lib.nflhip_any_eq_dev(self.ctx, _vp(a), _vp(b), self._batch(a), C.byref(r), self._stream(stream)))
        return bool(r.value)

    def any_neq(self, a, b, stream=None):
        r = C.c_int(0)
        self._chk(self.lib.nflhip_any_neq_dev(self.ctx, _vp(a), _vp(b), self._batch(a), C.byref(r), self._stream(stream)))
        return bool(r.value)

    def broadcast(self, one, count, stream=None):
        """`count` copies of one polynomial (nflhip_broadcast_dev)"""
        out = self.empty(count)
        self._chk(self.lib.nflhip_broadcast_dev(self.ctx, _vp(out), _vp(one), count, self._stream(stream)))
        return out

    def fill_uniform(self, d, seed, operand=0, first_poly=0, stream=None):
        self._chk(self.lib.nflhip_fill_uniform_dev(self.ctx, _vp(d), first_poly, self._batch(d), seed, operand,
                                                   self._stream(stream)))
        return d

    # ---- samplers (include/nflhip.h "samplers"): key = 32 bytes, stream_id selects the keystream ----
    @staticmethod
    def _key(key):
        key = bytes(key)
        assert len(key) == 32, "the sampler key is 32 bytes"
        return C.create_string_buffer(key, 32)

    def _sid(self, stream_id):
        """A (key, stream_id, distribution) triple must never be used twice for values that must be independent (a
        public polynomial and the noise next to it): without an explicit id every call takes a fresh one."""
        if stream_id is None:
            stream_id = self._next_stream
            self._next_stream += 1
        return stream_id

    NARROW = True   # this engine knows the narrow draws (DIST_NARROW, gauss_create(draw_bits=32))

    def sample(self, d, dist, key, stream_id=None, param0=0, param1=1, first_poly=0, stream=None, narrow=False):
        """dist: DIST_UNIFORM | DIST_BOUNDED (param0 = upper bound, param1 = amplifier) | DIST_ZO (param0 = rho)
        | DIST_HWT (param0 = hamming weight); narrow (uniform only): keystream lanes of the limb width (NFLHIP_DIST_NARROW)"""
        dist |= _lib.DIST_NARROW if narrow else 0
        self._chk(self.lib.nflhip_sample_dev(self.ctx, _vp(d), first_poly, self._batch(d), dist, param0, param1,
                                             self._key(key), self._sid(stream_id), self._stream(stream)))
        return d

    def sample_seq(self, d, dist, key, first_stream_id, stream_id_stride=1, param0=0, param1=1, stream=None, narrow=False):
        """polynomial b = sample(one polynomial, stream id first_stream_id + b*stride) (nflhip_sample_seq_dev)"""
        dist |= _lib.DIST_NARROW if narrow else 0
        self._chk(self.lib.nflhip_sample_seq_dev(self.ctx, _vp(d), self._batch(d), dist, param0, param1, self._key(key),
                                                 first_stream_id, stream_id_stride, self._stream(stream)))
        return d

    def sample_gauss_seq(self, d, g, key, first_stream_id, stream_id_stride=1, amplifier=1, stream=None):
        self._chk(self.lib.nflhip_sample_gauss_seq_dev(self.ctx, _vp(d), self._batch(d), g, amplifier, self._key(key),
                                                       first_stream_id, stream_id_stride, self._stream(stream)))
        return d

    def random_words(self, nwords, key, stream_id=0, first_word=0, stream=None):
        t = _torch()
        out = t.empty((nwords,), dtype=t.int64, device="cuda:%d" % self.device)
        self._chk(self.lib.nflhip_random_words_dev(self.ctx, _vp(out), first_word, nwords, self._key(key), stream_id,
                                                   self._stream(stream)))
        return out

    def gauss_create(self, sigma, security=128, samples=None, center=0.0, draw_bits=64):
        """FastGaussianNoise(sigma, security, samples, center): returns a handle for sample_gauss / gauss_info;
        draw_bits = 32: the narrow draw (nflhip_gauss_set_draw_bits)"""
        h = C.c_void_p()
        self._chk(self.lib.nflhip_gauss_create(self.ctx, C.byref(h), float(sigma), int(security),
                                               int(samples if samples is not None else self.degree), float(center)))
        if draw_bits != 64:
            if self.lib.nflhip_gauss_set_draw_bits(h, int(draw_bits)) != 0:
                self.lib.nflhip_gauss_destroy(self.ctx, h)
                raise ValueError("draw_bits must be 64 or 32")
        return h

    def gauss_destroy(self, g):
        self._chk(self.lib.nflhip_gauss_destroy(self.ctx, g))

    def gauss_info(self, g):
        import numpy as np
        x_min, entries, words, bits, tail = C.c_longlong(), C.c_size_t(), C.c_int(), C.c_uint(), C.c_double()
        self._chk(self.lib.nflhip_gauss_info(g, C.byref(x_min), C.byref(entries), C.byref(words), C.byref(bits),
                                             C.byref(tail), None))
        tab = np.zeros((entries.value, words.value), dtype=np.uint64)
        self._chk(self.lib.nflhip_gauss_info(g, None, None, None, None, None, tab.ctypes.data_as(C.c_void_p)))
        return {"x_min": x_min.value, "entries": entries.value, "words": words.value, "bit_precision": bits.value,
                "tail": tail.value, "table": tab}

    def sample_gauss(self, d, g, key, stream_id=None, amplifier=1, first_poly=0, stream=None):
        self._chk(self.lib.nflhip_sample_gauss_dev(self.ctx, _vp(d), first_poly, self._batch(d), g, amplifier,
                                                   self._key(key), self._sid(stream_id), self._stream(stream)))
        return d

    def gauss_noise(self, g, count, key, stream_id=None, first_sample=0, stream=None):
        """raw signed samples (FastGaussianNoise::getNoise) as an int64 device tensor"""
        t = _torch()
        out = t.empty((count,), dtype=t.int64, device="cuda:%d" % self.device)
        self._chk(self.lib.nflhip_gauss_noise_dev(self.ctx, _vp(out), first_sample, count, g, self._key(key),
                                                  self._sid(stream_id), self._stream(stream)))
        return out

    def h_gauss_noise(self, g, count, key, stream_id=None):
        out = np.empty((count,), dtype=np.int64)
        self._chk(self.lib.nflhip_gauss_noise(self.ctx, out.ctypes.data_as(C.c_void_p), count, g, self._key(key),
                                              self._sid(stream_id)))
        return out

    def crt_lift(self, d, stream=None):
        t = _torch()
        batch = self._batch(d)
        out = t.empty((batch, self.degree, self.crt_limbs), dtype=t.int64, device=d.device)
        self._chk(self.lib.nflhip_crt_lift_dev(self.ctx, _vp(out), _vp(d), batch, self._stream(stream)))
        return out

    def crt_project(self, limbs, stream=None):
        batch, deg, L = limbs.shape
        assert deg == self.degree and limbs.is_contiguous()
        out = self.empty(batch)
        self._chk(self.lib.nflhip_crt_project_dev(self.ctx, _vp(out), _vp(limbs), L, batch, self._stream(stream)))
        return out

    # ---- the batch split (include/nflhip.h "multi-GPU") ----
    def digest(self, d, first_poly=0, stream=None):
        """shard-composable 64-bit digest of a resident batch (sharding.digest_words is its numpy statement)"""
        out = C.c_uint64(0)
        self._chk(self.lib.nflhip_digest_dev(self.ctx, _vp(d), first_poly, self._batch(d), C.byref(out), self._stream(stream)))
        return int(out.value)

    def time_polymul(self, c, a, b, iters, stream=None):
        ms = C.c_float(0)
        self._chk(self.lib.nflhip_time_polymul_dev(self.ctx, _vp(c), _vp(a), _vp(b), self._batch(a), iters,
                                                   self._stream(stream), C.byref(ms)))
        return ms.value

    # ---- host-pointer path (numpy in, numpy out): what the per-poly C++ surface calls ----
    def _hb(self, a):
        assert isinstance(a, np.ndarray) and a.dtype == self.np_dtype and a.flags.c_contiguous
        assert a.size % self.words_per_poly == 0
        return a.size // self.words_per_poly

    def h_ntt(self, a):
        out = a.copy()
        self._chk(self.lib.nflhip_ntt_fwd(self.ctx, _vp(out), self._hb(out)))
        return out

    def h_intt(self, a):
        out = a.copy()
        self._chk(self.lib.nflhip_ntt_inv(self.ctx, _vp(out), self._hb(out)))
        return out

    def h_pointwise(self, op, a, b=None, bprime=None):
        out = np.empty_like(a)
        self._chk(self.lib.nflhip_pointwise(self.ctx, op, _vp(out), _vp(a), _vp(b), _vp(bprime), self._hb(a)))
        return out

    def h_polymul(self, a, b, out=None):
        out = np.empty_like(a) if out is None else out
        self._chk(self.lib.nflhip_polymul(self.ctx, _vp(out), _vp(a), _vp(b), self._hb(a)))
        return out

    def h_any_eq(self, a, b):
        r = C.c_int(0)
        self._chk(self.lib.nflhip_any_eq(self.ctx, _vp(a), _vp(b), self._hb(a), C.byref(r)))
        return bool(r.value)

    def h_any_neq(self, a, b):
        r = C.c_int(0)
        self._chk(self.lib.nflhip_any_neq(self.ctx, _vp(a), _vp(b), self._hb(a), C.byref(r)))
        return bool(r.value)

    def h_crt_lift(self, a):
        batch = self._hb(a)
        out = np.zeros((batch, self.degree, self.crt_limbs), dtype=np.uint64)
        self._chk(self.lib.nflhip_crt_lift(self.ctx, _vp(out), _vp(a), batch))
        return out

    def h_crt_project(self, limbs):
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
        batch, deg, L = limbs.shape
        out = np.empty((batch, self.nmoduli, self.degree), dtype=self.np_dtype)
        self._chk(self.lib.nflhip_crt_project(self.ctx, _vp(out), _vp(limbs), L, batch))
        return out

    def table(self, which, cm):
        n = {TAB_PSI: 2 * self.degree, TAB_OMEGAS: 2 * self.degree, TAB_INVOMEGAS: 2 * self.degree, TAB_MODULUS: 1,
             TAB_INVDEGREE: 1}.get(which, self.degree)
        out = np.zeros(n, dtype=self.np_dtype)
        self._chk(self.lib.nflhip_get_table(self.ctx, which, cm, _vp(out), out.nbytes))
        return out

    def crt_constant(self, what, cm=0):
        buf = np.zeros(self.crt_limbs + 2, dtype=np.uint64)
        n = C.c_size_t(0)
        self._chk(self.lib.nflhip_get_crt_constant(self.ctx, what, cm, _vp(buf), buf.size, C.byref(n)))
        return int.from_bytes(buf[:n.value].tobytes(), "little")


def shard_range(total, nranks, rank):
    """(first, count) of rank's contiguous shard: nflhip_shard_range (no device needed)"""
    f, c = C.c_size_t(0), C.c_size_t(0)
    rc = _lib.lib.nflhip_shard_range(total, nranks, rank, C.byref(f), C.byref(c))
    if rc != 0:
        raise NflHipError(rc, _lib.lib.nflhip_last_error(None).decode())
    return int(f.value), int(c.value)


class Comm:
    """One process per GPU: the RCCL communicator of include/nflhip.h (nflhip_comm_*).  Rank 0 draws `Comm.unique_id()`
    and hands the 128 bytes to the other ranks out of band (bench.py: torch.distributed's broadcast)."""

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        rc = _lib.lib.nflhip_comm_unique_id(buf)
        if rc != 0:
            raise NflHipError(rc, _lib.lib.nflhip_last_error(None).decode())
        return bytes(buf)

    def __init__(self, engine, nranks, rank, unique_id):
        self.eng, self.lib = engine, _lib.lib
        h = C.c_void_p()
        idb = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(unique_id)
        rc = self.lib.nflhip_comm_create(C.byref(h), engine.ctx, nranks, rank, idb)
        if rc != 0:
            raise NflHipError(rc, self.lib.nflhip_last_error(None).decode())
        self.h, self.nranks, self.rank = h, nranks, rank

    def close(self):
        if getattr(self, "h", None):
            self.lib.nflhip_comm_destroy(self.h)
            self.h = None

    def _chk(self, rc):
        if rc != 0:
            raise NflHipError(rc, self.lib.nflhip_last_error(None).decode())

    def scatter(self, shard, full, total, root=0, stream=None):
        self._chk(self.lib.nflhip_scatter_dev(self.h, _vp(shard), _vp(full), total, root, self.eng._stream(stream)))
        return shard

    def gather(self, full, shard, total, root=0, stream=None):
        self._chk(self.lib.nflhip_gather_dev(self.h, _vp(full), _vp(shard), total, root, self.eng._stream(stream)))
        return full

    def barrier(self, stream=None):
        self._chk(self.lib.nflhip_comm_barrier(self.h, self.eng._stream(stream)))

    def allgather_u64(self, value, stream=None):
        out = (C.c_uint64 * self.nranks)()
        self._chk(self.lib.nflhip_comm_allgather_u64(self.h, value & ((1 << 64) - 1), out, self.eng._stream(stream)))
        return [int(v) for v in out]


def gauss_table(sigma, security=128, samples=1024, center=0.0):
    """The cumulative table of nflhip_gauss_create, built on the host (no device needed): dict like Engine.gauss_info."""
    from ._lib import load
    lib = load()
    x_min, entries, words, bits, tail = C.c_longlong(), C.c_size_t(), C.c_int(), C.c_uint(), C.c_double()
    rc = lib.nflhip_gauss_table(sigma, security, samples, center, C.byref(x_min), C.byref(entries), C.byref(words), C.byref(bits),
                                C.byref(tail), None, 0)
    if rc:
        raise NflHipError(rc, lib.nflhip_last_error(None).decode())
    tab = np.zeros((entries.value, words.value), dtype=np.uint64)
    rc = lib.nflhip_gauss_table(sigma, security, samples, center, None, None, None, None, None, tab.ctypes.data_as(C.c_void_p), tab.size)
    if rc:
        raise NflHipError(rc, lib.nflhip_last_error(None).decode())
    return {"x_min": x_min.value, "entries": entries.value, "words": words.value, "bit_precision": bits.value,
            "tail": tail.value, "table": tab}
