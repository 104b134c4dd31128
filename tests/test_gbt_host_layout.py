"""The groupbytrace store's scratch layouts (odigos_amd/csrc/gbt_layout.hpp),
read through the host seam osehost_gbt_layout and compared with the formulae
gbt_host.cpp carved by hand before there was a layout function per buffer,
restated here in Python: every offset, every part's bytes and the end, on each
side of every 256-byte rounding; no part overlapping another, every part
inside the end, the parts the kernels read as 64-bit on 8-byte boundaries.
No device.
"""
import ctypes as C
import itertools
import re
from pathlib import Path

import pytest

from odigos_amd import native

HPP = (Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc" / "kernels.hpp").read_text()
SORT_TILE = int(re.search(r"constexpr\s+uint32_t\s+kSortTile\s*=\s*(\d+)\s*;", HPP).group(1))

ADD, RELEASE, SORT, OTLP_RINGS, WDEV = range(5)
ADD_PARTS = ["slot_of", "flag", "rank", "strlen", "stroff", "attrset_map", "keys", "vals", "hres", "hscope", "hlen",
             "hoff", "res_ref", "scope_ref"]
N = [1, 59, 60, 61, 64, 4096, 4097]   # 60: where 4n + 16 crosses a 256-byte boundary
A = [0, 1, 60, 61]
SR = [1, 30, 31, 61]                  # 30: where 8R + 16 crosses
W = [1, 2, 61]


def up(x, a=256):
    return (x + a - 1) // a * a


def seam(which, n=0, attrsets=0, scopes=0, resources=0, workers=1, otlp=0):
    off, nb, end = (C.c_uint64 * 32)(), (C.c_uint64 * 32)(), C.c_uint64()
    k = native.lib().osehost_gbt_layout(which, n, attrsets, scopes, resources, workers, otlp, off, nb, 32, C.byref(end))
    assert 0 < k <= 32
    return [(off[i], nb[i]) for i in range(k)], end.value


def chain(extents):
    """The hand carve: a part starts where the last one's extent ended."""
    offs, at = [], 0
    for e in extents:
        offs.append(at)
        at += e
    return offs, at


def check(got, end, want_offs, want_bytes, want_end, where):
    """got: the seam's (offset, bytes) per part; a part the store does not have is empty, wherever it is."""
    assert len(got) == len(want_offs), where
    for k, (g, o, b) in enumerate(zip(got, want_offs, want_bytes)):
        if b is None:
            assert g[1] == 0, (where, k)
        else:
            assert g == (o, b), (where, k, g, (o, b))
    assert end == want_end, where
    at = 0   # no two parts share a byte, none passes the end
    for off, nb in sorted(got):
        assert off >= at, (where, got)
        at = off + nb
    assert at <= end, where
    assert all(off % 256 == 0 for off, nb in got if nb), where


@pytest.mark.parametrize("n", N)
def test_add_scratch(n):
    for a, s, r, w, otlp in itertools.product(A, SR, SR, W, (0, 1)):
        where = (n, a, s, r, w, otlp)
        got, end = seam(ADD, n, a, s, r, w, otlp)
        # gbt_add: slot_of (8n), flag, rank, strlen, stroff (4n each), the attribute-set map
        extents = [up(8 * n)] + 4 * [up(4 * n + 16)] + [up(4 * a + 16)]
        nbytes = [8 * n] + 4 * [4 * n + 16] + [4 * a + 16]
        # W > 1: the (worker, rank) pairs
        extents += 2 * [up(4 * n + 16) if w > 1 else 0]
        nbytes += 2 * [4 * n + 16 if w > 1 else None]
        # OTLP: four header-length parts, the staged ResourceSpans and ScopeSpans refs
        hdr = 4 * [4 * s + 16] + [8 * r + 16, 8 * s + 16]
        extents += [up(b) if otlp else 0 for b in hdr]
        nbytes += [b if otlp else None for b in hdr]
        offs, want_end = chain(extents)
        assert want_end == (up(8 * n) + 4 * up(4 * n + 16) + up(4 * a + 16) + (2 * up(4 * n + 16) if w > 1 else 0)
                            + (4 * up(4 * s + 16) + up(8 * r + 16) + up(8 * s + 16) if otlp else 0))
        check(got, end, offs, nbytes, want_end, where)
        # what gbt_kernel.hip reads as 64-bit
        for name in ("slot_of", "res_ref", "scope_ref"):
            assert got[ADD_PARTS.index(name)][0] % 8 == 0, (where, name)


@pytest.mark.parametrize("w", N)
def test_release_scratch(w):
    got, end = seam(RELEASE, w)
    offs, want_end = chain(6 * [up(4 * w + 16)])
    assert want_end == 6 * up(4 * w + 16)
    check(got, end, offs, 6 * [4 * w + 16], want_end, w)


@pytest.mark.parametrize("m", N + [SORT_TILE - 1, SORT_TILE + 1, 3 * SORT_TILE, 3 * SORT_TILE + 1])
def test_sort_buffer(m):
    t = (m + SORT_TILE - 1) // SORT_TILE
    got, end = seam(SORT, m)
    offs, want_end = chain(4 * [up(4 * m + 16)] + 2 * [up(1024 * t + 16)])
    assert want_end == 4 * up(4 * m + 16) + 2 * up(1024 * t + 16)
    check(got, end, offs, 4 * [4 * m + 16] + 2 * [1024 * t + 16], want_end, m)


@pytest.mark.parametrize("c", N + [1024])
def test_otlp_ring_columns(c):
    for sc in sorted(set(SR + [c])):
        got, end = seam(OTLP_RINGS, c, scopes=sc)
        offs, want_end = chain([up(4 * c + 16), up(8 * sc + 16)] + 2 * [up(4 * sc + 16)])
        assert want_end == up(4 * c + 16) + up(8 * sc + 16) + 2 * up(4 * sc + 16)
        check(got, end, offs, [4 * c + 16, 8 * sc + 16] + 2 * [4 * sc + 16], want_end, (c, sc))
        assert got[1][0] % 8 == 0   # hdr_off: 64-bit


@pytest.mark.parametrize("w", [2, 31, 32, 33, 60, 61, 1 << 20])
def test_worker_buffer(w):
    got, end = seam(WDEV, workers=w)
    offs, want_end = chain([up(8 * w)] + 2 * [up(4 * w + 16)])
    assert want_end == up(8 * w) + 2 * up(4 * w + 16)
    check(got, end, offs, [8 * w] + 2 * [4 * w + 16], want_end, w)


def test_unknown_layout():
    off, nb, end = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), C.c_uint64()
    assert native.lib().osehost_gbt_layout(5, 1, 1, 1, 1, 1, 0, off, nb, 4, C.byref(end)) == 0
