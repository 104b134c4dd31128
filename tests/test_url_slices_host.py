"""The slices of the forked refs form's plan and spans pass (kernels.hpp
url_slices, read through the HIP-free seam osehost_url_slices): consecutive
group ranges that cover the batch, each with its own range of the size
stage's kept partials, inside what the size scratch reserves."""
import ctypes as C

import pytest

from odigos_amd import native

MAX_SLICES = 8            # kernels.hpp kUrlMaxSlices
COPY_MAX_BLOCKS = 65536   # kernels.hpp kUrlCopyMaxBlocks: what the size scratch reserves
FORMS = {"in_order": 0, "staggered": 1}
KS = (1, 2, 3, 4, 8)


def slices(n_groups, k, form):
    out = (C.c_uint32 * 20)()
    native.lib().osehost_url_slices(n_groups, k, form, out)
    kk = int(out[0])
    g = [int(out[2 + j]) for j in range(MAX_SLICES + 1)]
    p = [int(out[3 + MAX_SLICES + j]) for j in range(MAX_SLICES + 1)]
    return kk, int(out[1]), g, p


def _group_counts(k):
    return sorted({0, 1, 2, max(k - 1, 0), k, k + 1, 1000, 1_562_500})


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", KS)
def test_slices_cover_the_groups(k, form):
    for n in _group_counts(k):
        kk, reserved, g, p = slices(n, k, FORMS[form])
        assert kk == k
        assert reserved == COPY_MAX_BLOCKS
        assert g[0] == 0 and g[k] == n
        assert all(g[j] <= g[j + 1] for j in range(k)), (n, g)          # consecutive and disjoint
        assert all(x == n for x in g[k:]) and all(x == p[k] for x in p[k:])
        empty = [j for j in range(k) if g[j] == g[j + 1]]
        if n >= k:
            assert not empty, (n, k, g)
        # each slice's partials follow the slice before it; a slice with groups has at least one
        assert p[0] == 0
        for j in range(k):
            assert p[j + 1] >= p[j]
            if k > 1:
                assert (p[j + 1] > p[j]) == (g[j + 1] > g[j]), (n, k, j, g, p)
                # no more workgroups than the slice has pairs of groups per wave
                assert p[j + 1] - p[j] <= (g[j + 1] - g[j] + 7) // 8
        assert p[k] <= reserved


@pytest.mark.parametrize("form", sorted(FORMS))
def test_one_slice_is_the_batch(form):
    for n in (0, 1, 63, 1000, 1_562_500, 40_000_000):
        kk, reserved, g, p = slices(n, 1, FORMS[form])
        assert kk == 1 and g[:2] == [0, n] and p[0] == 0
        assert p[1] == max(1, min(COPY_MAX_BLOCKS, (n + 7) // 8)) <= reserved   # url_copy_blocks


@pytest.mark.parametrize("k", (2, 3, 4, 8))
def test_staggered_first_slice_is_half(k):
    n = 1_562_500
    _, _, g, _ = slices(n, k, FORMS["staggered"])
    sizes = [g[j + 1] - g[j] for j in range(k)]
    assert all(abs(s - sizes[1]) <= 1 for s in sizes[1:])
    assert abs(2 * sizes[0] - sizes[1]) <= 2
    _, _, g, _ = slices(n, k, FORMS["in_order"])
    sizes = [g[j + 1] - g[j] for j in range(k)]
    assert max(sizes) - min(sizes) <= 1


def test_rule():
    # K = 0 asks for the rule's slices: none below 2^20 groups (3M, 10M and 30M
    # spans lose or gain nothing sliced), two staggered ones from there up
    for n in (0, 1, 1000, 16384, 46875, 156_250, 468_750, (1 << 20) - 1, 1 << 20, 1_562_500, 40_000_000):
        kk, reserved, g, p = slices(n, 0, 0)
        assert kk == (2 if n >= 1 << 20 else 1), n
        assert g[kk] == n and p[kk] <= reserved
        if kk == 2:
            assert slices(n, 2, FORMS["staggered"])[2] == g and g[1] == (n + 2) // 3
