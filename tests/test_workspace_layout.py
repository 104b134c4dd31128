"""The stage workspaces' layouts (sampling_layout, url_layout, stage_offsets,
Engine::workspace_bytes), read through their host seams and compared with
the formulae the hosts carved by hand before there was a layout function per
stage, restated here in Python: every offset on each side of every rounding,
no part overlapping another, every part inside the layout's end.  No device.
"""
import ctypes as C
import itertools
import re
from pathlib import Path

import pytest

from odigos_amd import native

CSRC = Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc"
HPP = (CSRC / "kernels.hpp").read_text()


def const(name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\w+)\s*;" % name, HPP)
    assert m, f"{name}: definition not found"
    v = m.group(1)
    if not v.isdigit():   # a macro with a default (#define OSE_LONG_PIECE 2048)
        v = re.search(r"#define\s+%s\s+(\d+)" % v, HPP).group(1)
    return int(v)


SORT_TILE, SCAN_TILE = const("kSortTile"), const("kScanTileItems")
LONG_PIECE, LONG_PART = const("kLongPiece"), const("kLongPartBytes")
URL_GROUP, URL_SCAN_TILE = const("kUrlGroup"), const("kUrlScanTile")
URL_MAX_WAVES, URL_WAVE_SLACK, NFA_MAX_WAVES = const("kUrlMaxWaves"), const("kUrlWaveSlack"), const("kUrlNfaMaxWaves")
COPY_MAX_BLOCKS = const("kUrlCopyMaxBlocks")


def up(x, a=256):
    return (x + a - 1) // a * a


def ceil_div(a, b):
    return (a + b - 1) // b


def seam_parts(fn, *args):
    off, nb, end = (C.c_uint64 * 32)(), (C.c_uint64 * 32)(), C.c_uint64()
    k = fn(*args, off, nb, 32, C.byref(end))
    assert 0 < k <= 32
    return [(off[i], nb[i]) for i in range(k)], end.value


def check_disjoint_inside(parts, end, floor):
    """No two parts share a byte, none starts below `floor` or ends past `end`."""
    at = floor
    for off, nb in sorted(parts):
        assert off >= at, (parts, off, at)
        at = off + nb
    assert at <= end


# ---------------------------------------------------------------------------
# the trace stage

TRACE_PARTS = ["win_heads", "win_base", "wstatus", "rec", "key", "k2", "v2", "k3", "v3", "hist", "hoff", "hstatus",
               "long_runs", "long_meta", "long_pieces", "long_part", "win_first"]


def trace_sizes(n):
    W, N = max(1, ceil_div(n, 64)), max(n, 1)
    T = ceil_div(N, SORT_TILE)
    wtiles, htiles = ceil_div(W, SCAN_TILE), ceil_div(256 * T, SCAN_TILE)
    piece_cap = N // 64 + 1 + N // LONG_PIECE + 1
    part_cap = 2 * (N // LONG_PIECE) + 2
    return [8 * W, 4 * W, 8 * wtiles, 16 * N, 4 * N, 4 * N, 4 * N, 4 * N, 4 * N, 4 * 256 * T, 4 * 256 * T, 8 * htiles,
            4 * (N // 64 + 1), 16 * (N // 64 + 1), 8 * piece_cap, LONG_PART * part_cap, 8 * W]


def trace_layout_by_hand(n):
    """run_sampling_pass's take(): a part starts where the cursor is, the cursor
    moves to the next multiple of 256 past it; 256 bytes of words first, 256
    spare bytes last."""
    off, parts = 256, []
    for nb in trace_sizes(n):
        parts.append((off, nb))
        off = up(off + nb)
    return parts, off + 256


def around(m):
    return [m - 1, m, m + 1]


TRACE_N = sorted(set(
    [0, 1, 63, 64, 65]
    + around(64 * 2) + around(64 * 4)                                  # the window size
    + around(SORT_TILE) + around(3 * SORT_TILE)                        # the sort tile
    + around(64 * SCAN_TILE) + [64 * (SCAN_TILE - 1), 64 * (SCAN_TILE + 1)]   # the scan tile, in windows
    + around(64 * 2 * SCAN_TILE)
    # the scan tile in histogram entries: 256 per sort tile, so a multiple of SCAN_TILE / 256 sort tiles
    + around((SCAN_TILE // 256) * SORT_TILE) + around((SCAN_TILE // 256 - 1) * SORT_TILE)
    + around(2 * (SCAN_TILE // 256) * SORT_TILE)
    + around(LONG_PIECE) + around(3 * LONG_PIECE)))


@pytest.mark.parametrize("n", TRACE_N)
def test_trace_layout(n):
    got, end = seam_parts(native.lib().osehost_sampling_layout, n)
    want, want_end = trace_layout_by_hand(n)
    assert len(got) == len(TRACE_PARTS)
    for name, g, w in zip(TRACE_PARTS, got, want):
        assert g == w, (name, g, w)
    assert end == want_end
    assert all(off % 256 == 0 for off, _ in got) and end % 256 == 0
    check_disjoint_inside(got, end, floor=256)


# ---------------------------------------------------------------------------
# the URL stage

URL_PARTS = ["zero", "bump", "slow_aligned", "scan_status", "len", "meta", "code", "gsum", "gbase", "gscr", "slow",
             "unpl", "dbg", "scr", "slab"]


def url_scratch_bytes(n, arena):
    g = ceil_div(n, URL_GROUP)
    return ((arena + n + (arena + n) // 4 + 15) & ~15) + min(g, URL_MAX_WAVES) * URL_WAVE_SLACK


def url_nfa_slab_bytes(n, words):
    waves = min((ceil_div(n, URL_GROUP) + 3) & ~3, NFA_MAX_WAVES)
    return 256 + waves * 2 * words * URL_GROUP * 4 if words else 0


def url_layout_by_hand(n, arena, words, refs):
    """run_url's carve, offset by offset."""
    g = ceil_div(n, URL_GROUP)
    t = ceil_div(g, URL_SCAN_TILE)
    zero_bytes = 32 + 8 * t
    scr_bytes = 0 if refs else url_scratch_bytes(n, arena)
    o = {"zero": (0, zero_bytes), "bump": (16, 8), "slow_aligned": (24, 8), "scan_status": (32, 8 * t)}
    o["len"] = (up(zero_bytes), 4 * n)
    o["meta"] = (o["len"][0] + 4 * n, 4 * n)
    o["code"] = (up(o["meta"][0] + 4 * n, 8), 8 * n)
    o["gsum"] = (o["code"][0] + 8 * n, 8 * g)
    o["gbase"] = (o["gsum"][0] + 8 * g, 8 * g)
    o["gscr"] = (o["gbase"][0] + 8 * g, 8 * g)
    o["slow"] = (o["gscr"][0] + 8 * g, 4 * g)
    o["unpl"] = (o["slow"][0] + 4 * g, 4 * g)
    o["dbg"] = (up(o["unpl"][0] + 4 * g), 256)
    o["scr"] = (o["dbg"][0] + 256, scr_bytes)
    slab = up(o["scr"][0] + scr_bytes)
    o["slab"] = (slab, url_nfa_slab_bytes(n, words) - 256) if words else None
    end = slab + url_nfa_slab_bytes(n, words) - 256 if words else o["scr"][0] + scr_bytes
    return o, end


def url_closed_form(n, arena, words):
    g = ceil_div(n, URL_GROUP)
    t = ceil_div(g, URL_SCAN_TILE)
    return 16 + t * 8 + 256 + n * 16 + 8 + g * 32 + 512 + 256 + url_scratch_bytes(n, arena) + url_nfa_slab_bytes(n, words)


URL_N = [0, 1, 64, 65, 64 * 1024, 64 * 1024 + 1, 64 * 4096, 64 * 4096 + 1]
URL_ARENA = [0, 1, 15, 16, 2 ** 20]
URL_WORDS = [0, 1, 3]


def url_seam(n, arena, words, refs):
    ws = C.c_uint64()
    off, nb, end = (C.c_uint64 * 32)(), (C.c_uint64 * 32)(), C.c_uint64()
    k = native.lib().osehost_url_layout(n, arena, words, refs, off, nb, 32, C.byref(end), C.byref(ws))
    assert k == len(URL_PARTS)
    return {name: (off[i], nb[i]) for i, name in enumerate(URL_PARTS)}, end.value, ws.value


@pytest.mark.parametrize("n", URL_N)
def test_url_layout(n):
    for arena, words, refs in itertools.product(URL_ARENA, URL_WORDS, (0, 1)):
        got, end, ws_bytes = url_seam(n, arena, words, refs)
        want, want_end = url_layout_by_hand(n, arena, words, refs)
        where = (n, arena, words, refs)
        for name in URL_PARTS:
            if want[name] is None:   # no NFA program: an empty slab, wherever
                assert got[name][1] == 0, (where, name)
            else:
                assert got[name] == want[name], (where, name, got[name], want[name])
        assert end == want_end, where
        # the words one memset clears hold the refs words and the scan status, apart
        zb = got["zero"][1]
        check_disjoint_inside([got[k] for k in ("bump", "slow_aligned", "scan_status")], zb, floor=16)
        assert got["zero"][0] == 0
        check_disjoint_inside([got[k] for k in URL_PARTS[4:]], end, floor=zb)
        assert got["len"][0] % 256 == 0 and got["code"][0] % 8 == 0 and got["dbg"][0] % 256 == 0
        assert got["scr"][0] % 256 == 0 and (not words or got["slab"][0] % 256 == 0)
        # url_workspace_bytes: the non-refs layout's end, never above the closed form it replaces
        assert ws_bytes == url_layout_by_hand(n, arena, words, 0)[1], where
        assert end <= ws_bytes <= url_closed_form(n, arena, words), where


# ---------------------------------------------------------------------------
# the stages of one call

SAMPLE, TEMPLATE, SIZE = native.STAGE_SAMPLE, native.STAGE_TEMPLATE, native.STAGE_SIZE


def size_scratch_bytes(n_scopes):
    S = max(n_scopes, 1)
    W = ceil_div(S, 64)
    parts = up(256 + 8 * S)
    fix = up(parts + 32 * W)
    partials = up(fix + 4 * W)
    return up(partials + 4 * COPY_MAX_BLOCKS) + 256


def stage_offsets_by_hand(mask, defer, n, scopes, arena, words):
    """run_stages' chain."""
    samp = trace_layout_by_hand(n)[1]
    uws = url_layout_by_hand(n, arena, words, 0)[1]
    need = samp if mask & SAMPLE else 0
    url_off = up(samp if defer else 256) if mask & SAMPLE else 0
    size_off = 256 if mask & SAMPLE else 0
    if mask & TEMPLATE:
        need = max(need, url_off + uws)
        size_off = up(url_off + uws)
    if mask & SIZE:
        need = max(need, size_off + size_scratch_bytes(scopes))
    return url_off, size_off, need


def workspace_bytes_by_hand(mask, n, arena, words):
    """Engine::workspace_bytes' chain, every stage of `mask` configured."""
    s = up(trace_layout_by_hand(n)[1]) if mask & SAMPLE else 0
    if mask & TEMPLATE:
        s = up(s + url_layout_by_hand(n, arena, words, 0)[1])
    if mask & SIZE:
        s += size_scratch_bytes(n)
    return s


@pytest.mark.parametrize("n", URL_N)
def test_stage_offsets_and_workspace_bytes(n):
    out = (C.c_uint64 * 4)()
    for mask, defer, arena, words in itertools.product(range(8), (0, 1), URL_ARENA, (0, 3)):
        for scopes in sorted({0, 1, 64, 65, n}):
            native.lib().osehost_stage_offsets(mask, defer, n, scopes, scopes, arena, words, out)
            where = (mask, defer, n, scopes, arena, words)
            assert tuple(out[:3]) == stage_offsets_by_hand(mask, defer, n, scopes, arena, words), where
            assert out[0] % 256 == 0 and out[1] % 256 == 0, where
            assert out[3] == workspace_bytes_by_hand(mask, n, arena, words), where
