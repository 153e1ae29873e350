"""CPU: the chunk geometry of the NTT-form permutation kernels (k_permute_add_ntt, k_permute_mac_ntt, the several-output kernel), which
cut a row longer than kNttChunkBytes into 2^c chunks and rely on sigma_k mapping chunks to chunks.  The index map of
nfllib_amd/csrc/automorph_index.h restated in Python, checked for every chunk count -- and the reason why
tests/test_gpu_long_rows.py runs rows of 8 chunks and more with the multipliers 3 and 5."""
import numpy as np
import pytest

from automorph_util import ntt_source, rev


def aut_ntt_src(j, k, logn):
    """automorph_index.h aut_ntt_src restated, 32-bit wrap included: rev(((k (2 rev(j) + 1)) & (2n - 1)) >> 1)"""
    t = ((k & 0xFFFFFFFF) * (2 * rev(j, logn) + 1)) & 0xFFFFFFFF
    return rev((t & ((2 << logn) - 1)) >> 1, logn)


def aut_inverse_mod_2n(k, logn):
    """automorph_index.h aut_inverse_mod_2n restated: five Newton steps on 32-bit words"""
    x = k
    for _ in range(5):
        x = (x * ((2 - k * x) & 0xFFFFFFFF)) & 0xFFFFFFFF
    return x & ((2 << logn) - 1)


def chunk_map(src, logn, c):
    """source chunk per destination chunk with 2^c chunks a row, from src = aut_ntt_src of every slot; asserts that every destination
    chunk has exactly one"""
    blocks = (src >> (logn - c)).reshape(1 << c, -1)
    assert (blocks == blocks[:, :1]).all(), (logn, c)
    return blocks[:, 0]


def _odd_spread(n):
    """every odd k below 2n for the short rows; otherwise the small ones, the ones around n and 2n, powers of 5 and random ones"""
    if n <= 64:
        return list(range(1, 2 * n, 2))
    rnd = np.random.RandomState(n)
    ks = {1, 3, 5, 7, 9, 15, 17, n - 1, n + 1, 2 * n - 1, 2 * n - 3, 2 * n - 5, pow(5, 7, 2 * n), pow(5, n // 4 - 1, 2 * n), (2 * n - 1) * 25 % (2 * n)}
    return sorted(ks | {int(x) * 2 + 1 for x in rnd.randint(0, n, size=4)})


@pytest.mark.parametrize("logn", range(4, 17))
def test_chunks_map_to_chunks_and_the_inverse_multiplier_maps_them_back(logn):
    """what the three kernels lean on, for every chunk count 2^c <= n / 2: sigma_k fills each destination chunk from exactly ONE
    source chunk (the mac kernels look that chunk up through k), and the image of that source chunk's first slot under k^-1 lies in
    the destination chunk (k_permute_add_ntt finds its output chunk that way).  The restated index map is the numpy one of
    tests/automorph_util.py, and the restated inverse is an inverse."""
    n = 1 << logn
    for k in _odd_spread(n):
        kinv = aut_inverse_mod_2n(k, logn)
        assert k * kinv % (2 * n) == 1, (n, k)
        by_k, by_kinv = aut_ntt_src(np.arange(n), k, logn), aut_ntt_src(np.arange(n), kinv, logn)
        assert np.array_equal(by_k, ntt_source(n, k)), (n, k)
        for c in range(1, logn):
            src = chunk_map(by_k, logn, c)
            assert sorted(src.tolist()) == list(range(1 << c)), (n, k, c)                  # a permutation of the chunks
            back = aut_ntt_src(src << (logn - c), kinv, logn) >> (logn - c)                # first slot of each source chunk, by k^-1
            assert np.array_equal(back, np.arange(1 << c)), (n, k, c)
            assert np.array_equal(chunk_map(by_kinv, logn, c)[src], np.arange(1 << c)), (n, k, c)


@pytest.mark.parametrize("logn", range(4, 17))
def test_k_and_its_inverse_share_the_chunk_map_up_to_four_chunks_and_not_at_eight(logn):
    """the chunk index is bits 1 .. c of the odd exponent, so the chunk map of k depends on k mod 2^(c + 1) only, and k^2 = 1 (mod 8) for
    every odd k: with 2 or 4 chunks a k in the place of k^-1 cannot show.  With 8 chunks it shows exactly when k^2 != 1 (mod 16): for
    k = 3 and 5, not for 7, 9, 15 or 2n - 1."""
    n = 1 << logn

    def maps(k, c):
        return chunk_map(aut_ntt_src(np.arange(n), k, logn), logn, c), chunk_map(aut_ntt_src(np.arange(n), aut_inverse_mod_2n(k, logn), logn), logn, c)
    for k in _odd_spread(n):
        for c in (1, 2):
            assert np.array_equal(*maps(k, c)), (n, k, c)
        assert np.array_equal(*maps(k, 3)) == (k * k % 16 == 1), (n, k)
    for k in (3, 5):
        assert not np.array_equal(*maps(k, 3)), (n, k)
    for k in (7, 9, 15, 2 * n - 1):
        assert np.array_equal(*maps(k, 3)), (n, k)
