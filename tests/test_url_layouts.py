"""The URL stage on hand-laid batches: one named layout per seam of
url_plan_kernel, url_plan_slow_kernel, url_emit_slow_kernel and
url_copy_kernel, each compared with the oracle bit for bit
(tests/url_layouts.py builds them).

The generator's paths hold 1-6 short segments and reach these seams by chance,
if at all; here every layout's census (computed from the built columns alone)
first proves that the batch holds its seam, the C oracle is pinned against a
pure-Python restatement on it, and then the HIP stage must give the oracle's
url_out, template refs and bytes, in the packed and the refs form, under the
default instance and under url_plan_kernel<1> (a config whose one custom id
and one 40-segment rule match nothing).

Layout               guards (constant / code line)
-------------------  ----------------------------------------------------------
stage.3072 / 3073    kPlanStage (3072), stage_dma `bytes <= kPlanStage`: 64
                     paths of 48 bytes from a 16-aligned offset, the last one
                     ending on the stage's last byte in a 1-byte segment (the
                     `rd.word(s + 16)` over-read of the +16 padding); moved up
                     one byte: range 3088, 256 chunks, unplanned
gather.fit / over1   `total * 16 > kPlanStage`: 64 paths at a 64-byte pitch, 192
                     chunks (16-aligned, and off & 15 == 15 with shorter
                     paths); one path of 49 bytes: 193 chunks
gather.sparse        the binary search over the chunk scan: paths in lanes 0,
                     31, 32 and 63 only, megabytes apart, gate 0 / gate 1 /
                     len == 0 lanes between them
gather.rounds        the 1 KB DMA rounds (`64 * k < total`): 64, 65, 128, 129
                     chunks
slow.subsets         url_plan_slow_kernel `cs + nc <= kPlanStage / 16`: 2 and 3
                     subsets, each full one ending exactly at 192 chunks
slow.alone           `alone`, plan_global: a path of kPlanStage + 28 bytes in
                     lane 0 of one group and lane 63 of another
slow.alone4k         kStage (4096), stage_wave `bytes > kStage`: a path over 4
                     KB, url_emit_slow_kernel's ByteReader branch
slow.img4096         kWaveOut (4096), `img_bytes > kWaveOut`: slow-listed groups
                     with shift + sum of 4096 (shift 0 and 1) and 4097 (direct)
win.192/193          `b0 + plen <= 192` for b0 in {0, 31}
slash.halves         half_mask / the sl0..sl2 loops: the last slash at window
                     bits 63, 64, 127, 128, 191; "////"; a trailing slash; no
                     leading slash, templated and untouched (processor.go:182)
qm                   the '?' cut (q0..q2, first_of): n = 0 and 1, '?' at window
                     bits 63, 64, 127, 128, past bit 192 in a non-window path,
                     two '?', none, a '/' after it; the same bytes as PATH_RAW
segcap.192/193       kSegCap (192) `total > kSegCap`; 64, 65, 128, 129 entries
                     (the classify and assembly steps of 64, `carry`)
seg.64/65            `L <= 64`: a 64-byte segment that stays, 64 hex digits, a
                     65-byte one (`longseg`), starting at row bits 0, 1, 31
fold.8/9             `nseg <= 8`, `k < 16 && id < 15`: nseg 1, 7, 8, 9, 16, 17
                     with the id first, last, at 7, 8, 15, 16; 16 and 17 also in
                     groups over kImgCap (p.code, p.slow, emit_path)
gates                plan_gate: gate 0 (no method, internal, target present),
                     gate 1 (a lone "/" and RENAME), gate 2 with len == 0 and
                     with NAME_EQ_METHOD; an all-gate-0 group (`lo >= hi`,
                     sum == 0, {0, 0} refs) between two full ones
date, hex, digits,   classify_spec / classify_win (date_flat / date_win,
uuid, email,         email_flat / email_win, has_fffd_win): every case at row
noletters, fffd      bits 0, 1, 31, as a path's last segment with the byte that
                     would flip it laid right after, and as a middle segment
asm.tails            assemble_group's `nf`, `rem` and overlapping stores:
                     untouched segments of 1-17 bytes, {id}, {date}, {email} at
                     every output offset mod 8, the next path's bytes after each
img.cap/over         kImgCap (4752) `sum <= kImgCap`: sums 4751, 4752, 4753
copy.tiny            url_copy_kernel's bytewise stores: consecutive group sums
                     of 1, 1, 1, 1, 2, 3, 0, 5 (several groups per dword), then
                     every base & 3
copy.rounds          copy_round's `carry`: n16 == 64 with nchunk == 65, 128 /
                     129, shift > 0
names.15/16          the braced table (ids 0..14) and `big`: custom ids with
                     name ids 13, 14, 15
names.64/65          kNameTab (64), name_len_global: name ids 63, 64
names.254/255        `id + 1` saturating at 255: name ids 253, 254, 255
names.braced         kBNames / `l > 255`: load_braced_names gives up, fused_cfg
                     is false and every group takes the per-span writer
dirty.then.seam      stale LDS between a wave's consecutive groups (row_bits,
                     load_win6, first_of, count_of reading rows r + 1, r + 2):
                     kUrlMaxWaves dirty groups (a full stage of '/', '?', '@',
                     digits, 0xFF; 192 segments; an image within 16 bytes of
                     kImgCap, so it covers every bitmap row it overlays), then
                     kUrlMaxWaves groups
                     cycling through every enumeration, classification and
                     assembly seam group, so whatever the plan grid's stride
                     each wave takes a seam group after a dirty one

The witness: with the engine option "url_path_counts" on,
Engine.path_counts()["url_unplanned"] is the number of groups
url_plan_slow_kernel planned in the call and ["url_slow"] the number
url_emit_slow_kernel emitted; both must equal Layout.expect() (url_slow only
for batches of at most kUrlMaxWaves groups: beyond that a wave's scratch
region, or in the refs form the order of the waves' atomics, may refuse an
image, which changes who writes a group but not a byte of the result).  In the
refs form `used` depends on the order of the waves' chunk reservations; it is
asserted within the bound tests/test_url_refs.py states.

refs.chunk           url_refs_chunk, `csz = max(a.refs_chunk, need)`: refs form
                     with a tmpl_cap that makes a wave's chunk 1024 bytes;
                     images of 1024, 1023, 1009 (the chunk ends exactly at the
                     image), 1008 and 1025 bytes (one byte past it).  Eight
                     groups or fewer, so the plan grid is one wave per group on
                     any device
"""
import copy
import ctypes as C

import numpy as np
import pytest

from odigos_amd import native
from tests import url_layouts as ul
from tests.oracle_lib import UrlOracle, size_process, span_template_bytes
from tests.url_layouts import K, WAVE

CPU_NAMES = ul.DEFAULT_NAMES
SMALL = [n for n in ul.DEFAULT_NAMES if n != ul.DIRTY]
REFS = native.STAGE_TEMPLATE_REFS


def test_constants_as_designed():
    # the layouts were drawn for these values: retuning one moves a seam, and
    # the layouts (and the table in this module's docstring) move with it
    got = {k: getattr(K, k) for k in ul.DESIGNED}
    assert got == ul.DESIGNED, "a URL-stage constant changed: re-lay tests/url_layouts.py against it"
    assert K.kImgCap == K.kRowVec * K.kPlanBmRows * 16 and K.kUrlWaveSlack > K.kImgCap > K.kWaveOut


# ---------------------------------------------------------------------------
# census: each layout holds its seam (from the built columns alone)

def _lane(L, seam):
    r = L.find(seam)
    assert len(r) == 1, (seam, r)
    return r[0]


def _d(L, seam):
    g, j = _lane(L, seam)
    return L.dispatch()[g], j


def census_stage(L, shift):
    d, j0 = _d(L, "p0")
    _, j63 = _d(L, "p63")
    assert d.needs == WAVE and (d.lo & 15) == shift
    assert d.hi - d.lo == K.kPlanStage and d.segs[j63][-1] == 1          # ends in a 1-byte segment
    if shift == 0:
        assert d.range_bytes == K.kPlanStage and d.staging == "contiguous" and d.listed
        assert int(d.p0[j63]) + int(L.path[_lane(L, "p63")[0] * WAVE + j63, 1]) == K.kPlanStage    # the stage's last byte
        assert d.total == K.kSegCap
    else:
        assert d.range_bytes == K.kPlanStage + 16 and d.chunks == 256 and d.staging == "unplanned" and d.unplanned


def census_gather(L, over):
    da, _ = _d(L, "a0")
    db, _ = _d(L, "b0")
    assert da.range_bytes > K.kPlanStage and db.range_bytes > K.kPlanStage
    assert da.chunks == K.kPlanStage // 16 + over and db.chunks == K.kPlanStage // 16
    assert da.staging == ("unplanned" if over else "gathered") and db.staging == "gathered" and db.listed
    g = _lane(L, "b0")[0]
    assert ((L.path[g * WAVE:(g + 1) * WAVE, 0] & 15) == 15).all()
    g = _lane(L, "a0")[0]
    assert ((L.path[g * WAVE:(g + 1) * WAVE, 0] & 15) == 0).all()


def census_sparse(L):
    d, _ = _d(L, "s0")
    assert d.staging == "gathered" and d.listed and d.range_bytes > (2 << 20)
    assert np.nonzero(d.nc)[0].tolist() == [0, 31, 32, 63]
    assert set(d.gate.tolist()) == {0, 1, 2} and ((d.gate == 2) & (d.nc == 0)).sum() >= 10       # len == 0 lanes


def census_rounds(L):
    for total in (64, 65, 128, 129):
        d, _ = _d(L, f"r{total}")
        assert d.staging == "gathered" and d.chunks == total and d.listed, (total, d.chunks, d.staging)


def census_subsets(L):
    full = K.kPlanStage // 16
    d, _ = _d(L, "two")
    assert d.unplanned and d.subsets == [("subset", 32, full), ("subset", 32, full)]
    d, _ = _d(L, "three")
    assert d.unplanned and d.subsets == [("subset", 24, full), ("subset", 24, full), ("subset", 16, 128)]


def census_alone(L, over):
    d, j = _d(L, "first")
    assert j == 0 and d.unplanned and d.subsets[0][:2] == ("alone", 0) and d.subsets[0][2] > K.kPlanStage // 16
    assert d.subsets[1][:2] == ("subset", WAVE - 1)
    d, j = _d(L, "last")
    assert j == WAVE - 1 and d.unplanned and d.subsets[0][:2] == ("subset", WAVE - 1) and d.subsets[1][:2] == ("alone", WAVE - 1)
    for seam in ("first", "last"):
        g, j = _lane(L, seam)
        assert over < int(L.path[g * WAVE + j, 1]) < over + 128


def census_img4096(L):
    sums = L.group_sums()
    base = np.cumsum(sums) - sums
    got = [(int(base[g] & 3), int((base[g] & 3) + sums[g])) for g in range(3)]
    assert got == [(0, K.kWaveOut), (0, K.kWaveOut + 1), (1, K.kWaveOut)], got
    assert all(L.dispatch()[g].unplanned for g in range(3))
    assert (sums[:3] <= K.kImgCap).all()        # slow-listed for the long segment alone


def census_win(L):
    for seam, b0, end in (("w192.0", 0, 192), ("w193.0", 0, 193), ("w192.31", 31, 192), ("w193.31", 31, 193)):
        d, j = _d(L, seam)
        g = _lane(L, seam)[0]
        assert d.staging == "contiguous" and d.listed
        assert int(d.p0[j]) & 31 == b0 and b0 + int(L.path[g * WAVE + j, 1]) == end and bool(d.win[j]) == (end <= K.win_bits)


def census_slash(L):
    for seam, bit in (("s63", 63), ("s64", 64), ("s127", 127), ("s128", 128), ("s191", 191)):
        d, j = _d(L, seam)
        g = _lane(L, seam)[0]
        p = L.path_bytes(g * WAVE + j)
        assert d.win[j] and int(d.p0[j]) & 31 == 0 and p.rfind(b"/") == bit, (seam, p.rfind(b"/"))
    d, j = _d(L, "only")
    assert d.segs[j] == [0, 0, 0, 0]
    d, j = _d(L, "trail")
    assert d.segs[j][-1] == 0
    d, j = _d(L, "nolead.t")
    assert d.lead[j] == 0
    _, tm = L.py_process()
    g, j = _lane(L, "nolead.t")
    assert tm[g * WAVE + j] == b"a/{id}"
    g, j = _lane(L, "nolead.u")
    assert tm[g * WAVE + j] == b"/a/b"


def census_qm(L):
    for seam, n in (("n0", 0), ("n1", 1), ("q63", 63), ("q64", 64), ("q127", 127), ("q128", 128), ("far", 250), ("two", 4),
                    ("slash", 2)):
        d, j = _d(L, seam)
        assert int(d.n[j]) == n and int(d.p0[j]) & 31 == 0, (seam, int(d.n[j]))
        assert bool(d.win[j]) == (seam != "far")
        r, jr = _d(L, seam + ".raw")
        g = _lane(L, seam)[0]
        assert int(r.n[jr]) == int(L.path[g * WAVE + j, 1]) > n and r is d
    d, j = _d(L, "none")
    assert int(d.n[j]) == 10
    for ln in (200, 223, 224, 225):       # no '?' in the path, one in the byte after it
        d, j = _d(L, f"far.none{ln}")
        g = _lane(L, f"far.none{ln}")[0]
        o = int(L.path[g * WAVE + j, 0])
        assert int(d.n[j]) == ln and not d.win[j] and int(d.p0[j]) & 31 == 0
        assert L.arena[o + ln:o + ln + 8].tobytes() == b"1234567?" and b"?" not in L.path_bytes(g * WAVE + j)
        assert ((ln + 7) // 32 == (ln - 1) // 32) == (ln in (200, 225))      # the '?' in first_of's last window
    assert all(x.listed for x in L.dispatch())


def census_segcap(L):
    for total in (64, 65, 128, 129, 192, 193):
        d, _ = _d(L, f"t{total}")
        assert d.total == total and d.staging == "contiguous" and d.listed == (total <= K.kSegCap)


def census_seg(L):
    for a in ul.ALIGN:
        for seam, ln, listed in ((f"stay@{a}", K.win_seg, True), (f"hex@{a}", K.win_seg, True), (f"long@{a}", K.win_seg + 1, False),
                                 (f"longnl@{a}", K.win_seg + 1, False)):
            d, j = _d(L, seam)
            assert d.staging == "contiguous" and d.segs[j] == [ln] and d.listed == listed
            assert (int(d.p0[j]) + 1) & 31 == a, (seam, int(d.p0[j]))
    assert int(L.dispatch()[_lane(L, "stay@0")[0]].longest.max()) == K.win_seg


def census_fold(L):
    seen = set()
    sums = L.group_sums()
    for n, t in ul.FOLD:
        r = L.find(f"f{n}.{t}")
        assert len(r) == (1 if n <= 9 else 2)
        for g, j in r:
            d = L.dispatch()[g]
            assert d.nseg[j] == n and d.listed and d.segs[j][t] == 7
            seen.add((n, bool(sums[g] > K.kImgCap)))
    assert seen == {(1, False), (7, False), (8, False), (9, False), (16, False), (17, False), (16, True), (17, True)}
    assert {n for n, _ in ul.FOLD} == {1, K.fold - 1, K.fold, K.fold + 1, K.code_nibbles, K.code_nibbles + 1}


def census_gates(L):
    want = {"nomethod": 0, "internal": 0, "tgt.str": 0, "tgt.nonstr": 0, "gate1": 1, "gate1.nopath": 1, "len0": 2, "len0.eq": 2,
            "eq": 2, "path.none": 0}
    d = L.dispatch()
    for seam, gate in want.items():
        for g, j in L.find(seam):
            assert g == 1 and d[g].gate[j] == gate, seam
    assert set(d[1].gate.tolist()) == {0, 1, 2}
    assert d[3].staging == "empty" and not d[3].gate.any() and L.group_sums()[3] == 0
    assert d[2].needs == WAVE and d[4].needs == WAVE


def census_classify(family):
    def check(L):
        d = L.dispatch()
        assert all(x.staging == "contiguous" and x.listed for x in d)
        for label, seg, _ in ul.CASES[family]:
            for a in ul.ALIGN:
                for sfx in ("", "m"):
                    g, j = _lane(L, f"{label}@{a}{sfx}")
                    p = L.path_bytes(g * WAVE + j)
                    at = p.index(b"/", 1) + 1
                    assert p[at:at + len(seg)] == seg and (int(d[g].p0[j]) + at) & 31 == a, (label, a)
                    assert (len(p) == at + len(seg)) == (sfx == "")
    return check


def census_tails(L):
    off, ln = L.lane_out_offsets()
    want = {f"u{k}": k + 1 for k in range(1, 18)}
    want.update(id=5, date=7, email=8)
    for seam, out in want.items():
        r = L.find(seam)
        assert {int(off[g * WAVE + j]) % 8 for g, j in r} == set(range(8)), seam
        assert {int(ln[g * WAVE + j]) for g, j in r} == {out}
    assert all(x.listed and x.staging == "contiguous" for x in L.dispatch())
    assert (L.group_sums() <= K.kImgCap).all()


def census_img(L):
    sums = L.group_sums()
    for seam, s in (("cap-1", K.kImgCap - 1), ("cap", K.kImgCap), ("cap+1", K.kImgCap + 1)):
        g = _lane(L, seam)[0]
        assert sums[g] == s and L.dispatch()[g].listed
    assert L.expect() == dict(url_unplanned=0, url_slow=1)


def census_tiny(L):
    sums = L.group_sums()
    assert sums[:len(ul.TINY)].tolist() == list(ul.TINY)
    base = np.cumsum(sums) - sums
    assert (base[:4] // 4 == 0).all()                 # four groups in one destination dword
    for lo in (8, 11):
        assert {int(b) & 3 for b, s in zip(base[lo:], sums[lo:]) if s} == {0, 1, 2, 3}, lo
    assert all(x.listed for x in L.dispatch())


def census_rounds_copy(L):
    sums = L.group_sums()
    base = np.cumsum(sums) - sums
    got = {((int(s) + 15) // 16, (int(b & 3) + int(s) + 15) // 16) for b, s in zip(base, sums) if b & 3}
    assert {(64, 65), (64, 64), (128, 129)} <= got, got
    assert (sums <= K.kImgCap).all() and all(x.listed for x in L.dispatch())


def census_refs_chunk(L):
    assert 4 < L.n_groups <= 8 and ul.refs_chunk(ul.REFS_CHUNK_CAP, L.n_groups) == ul.REFS_CHUNK
    assert ul.refs_chunk(ul.REFS_CHUNK_CAP - 64 * 16, L.n_groups) == ul.REFS_CHUNK - 16
    sums = L.group_sums()
    need = (sums + 15) & ~15
    got = {}
    for s in (1024, 1023, 1009, 1008, 1025):
        g = _lane(L, f"c{s}")[0]
        assert sums[g] == s and L.dispatch()[g].listed
        got[s] = int(need[g]) - ul.REFS_CHUNK
    assert got == {1024: 0, 1023: 0, 1009: 0, 1008: -16, 1025: 16}
    # the arena holds every wave's chunk (or, for the larger image, its need) with the bound's slack to spare
    assert int(np.maximum(need, ul.REFS_CHUNK).sum()) <= ul.REFS_CHUNK_CAP


def census_dirty(L):
    W = K.kUrlMaxWaves
    assert L.n == 2 * W * WAVE == 524_288 and L.n_groups == 2 * W
    d = L.dispatch()
    sums = L.group_sums()
    for g in (0, 1, 2, 3, W // 2, W - 2, W - 1):
        x = d[g]
        assert x.staging == "contiguous" and x.range_bytes == K.kPlanStage and x.total == K.kSegCap and x.listed
        # the image overlays the class bitmaps: it covers all kPlanBmRows rows of them, and no byte of it is zero
        assert K.kImgCap - 16 < sums[g] <= K.kImgCap and -(-int(sums[g]) // (16 * K.kRowVec)) == K.kPlanBmRows
        a = L.arena[x.lo:x.hi]
        assert all((a == c).sum() > 50 for c in b"/?@") and (a == 0xFF).sum() == 40 and ((a >= 48) & (a < 58)).sum() > 200
        assert x.needs == WAVE and (x.nseg == 3).all()
    url_out, refs, out_arena, used = L.oracle()
    first = int(sums[:W].sum())
    assert (out_arena[:first] != 0).all() and b"{id}" in out_arena[:int(sums[0])].tobytes()
    for g in (0, 1):
        assert L.dispatch()[g].listed
    assert (sums[:W] == sums[:2].tolist() * (W // 2)).all()
    k = len(L.kinds)
    assert k <= W and len(set(L.kinds)) == k
    # every seam kind within any k consecutive groups of the second half
    ref = ul.seam_kinds()
    for q in range(k):
        got, want = L.lanes[q * WAVE:(q + 1) * WAVE], ref[q][1]
        assert [x.path for x in got] == [x.path for x in want] and [x.seam for x in got] == [x.seam for x in want]
    assert [x.path for x in L.lanes[k * WAVE:(k + 1) * WAVE]] == [x.path for x in ref[0][1]]       # and round again


CENSUS = {
    "stage.3072": lambda L: census_stage(L, 0), "stage.3073": lambda L: census_stage(L, 1),
    "gather.fit": lambda L: census_gather(L, 0), "gather.over1": lambda L: census_gather(L, 1),
    "gather.sparse": census_sparse, "gather.rounds": census_rounds, "slow.subsets": census_subsets,
    "slow.alone": lambda L: census_alone(L, K.kPlanStage + 16), "slow.alone4k": lambda L: census_alone(L, K.kStage),
    "slow.img4096": census_img4096, "win.192/193": census_win, "slash.halves": census_slash, "qm": census_qm,
    "segcap.192/193": census_segcap, "seg.64/65": census_seg, "fold.8/9": census_fold, "gates": census_gates,
    **{f: census_classify(f) for f in ul.CASES},
    "asm.tails": census_tails, "img.cap/over": census_img, "copy.tiny": census_tiny, "copy.rounds": census_rounds_copy,
    "refs.chunk": census_refs_chunk,
    ul.DIRTY: census_dirty,
}

# what the witnesses must read (Layout.expect() computes it; pinned here so a
# layout that slides to another kernel is seen on the CPU)
EXPECT = {"stage.3072": (0, 0), "stage.3073": (1, 1), "gather.fit": (0, 0), "gather.over1": (1, 1), "gather.sparse": (0, 0),
          "gather.rounds": (0, 0), "slow.subsets": (2, 2), "slow.alone": (2, 2), "slow.alone4k": (2, 2), "slow.img4096": (3, 3),
          "win.192/193": (0, 0), "slash.halves": (0, 0), "qm": (0, 0), "segcap.192/193": (1, 1), "seg.64/65": (1, 1),
          "fold.8/9": (0, 2), "gates": (0, 0), "date": (0, 0), "hex": (0, 0), "digits": (0, 0), "uuid": (0, 0), "email": (0, 0),
          "noletters": (0, 0), "fffd": (0, 0), "asm.tails": (0, 0), "img.cap/over": (0, 1), "copy.tiny": (0, 0),
          "copy.rounds": (0, 0), "refs.chunk": (0, 0), "names.15/16": (0, 1), "names.64/65": (0, 2), "names.254/255": (0, 3), "names.braced": (0, 4)}


def test_every_layout_has_a_census():
    assert set(CENSUS) == set(ul.DEFAULT_NAMES) and set(EXPECT) == set(SMALL) | set(ul.NAMES)


@pytest.mark.parametrize("name", CPU_NAMES)
def test_census(name):
    L = ul.layout(name)
    CENSUS[name](L)
    if name in EXPECT:
        e = L.expect()
        assert (e["url_unplanned"], e["url_slow"]) == EXPECT[name]
        assert L.n_groups <= K.kUrlMaxWaves


@pytest.mark.parametrize("name", list(ul.NAMES))
def test_census_names(name):
    L = ul.layout(name)
    e = L.expect()
    assert (e["url_unplanned"], e["url_slow"]) == EXPECT[name]
    url_out, refs, arena, used = L.oracle()
    text = arena.tobytes()
    ids = sorted(int(s[2:]) for s in L.seams() if s.startswith("id") and "." not in s)
    for i in ids:       # the custom id matched where it should and nowhere else
        g, j = _lane(L, f"id{i}")
        o, l = refs[g * WAVE + j]
        name_i = b"n" * 254 if (name == "names.braced" and i == 3) else b"n%03d" % (i - 3)
        assert arena[o:o + l].tobytes() == b"/x/{" + name_i + b"}/y"
        g, j = _lane(L, f"id{i}.near")
        o, l = refs[g * WAVE + j]
        assert b"{" not in arena[o:o + l].tobytes()
    want = {"names.15/16": [13, 14, 15], "names.64/65": [K.kNameTab - 1, K.kNameTab], "names.254/255": [253, 254, 255],
            "names.braced": [3, 4]}[name]
    assert ids == want and text.count(b"{n") == 2 * len(ids)
    assert L.fused == (name != "names.braced")


def _perturbed(name, edit):
    L = copy.copy(ul.layout(name))
    L.arena, L.path = L.arena.copy(), L.path.copy()
    L._dispatch = L._oracle = None
    edit(L)
    L._bind()
    return L


def _set_len(seam, by):
    def edit(L):
        g, j = _lane(L, seam)
        L.path[g * WAVE + j, 1] = int(L.path[g * WAVE + j, 1]) + by
    return edit


def _slash_in(seam, at):
    def edit(L):
        g, j = _lane(L, seam)
        L.arena[int(L.path[g * WAVE + j, 0]) + at] = ord("/")
    return edit


@pytest.mark.parametrize("name,edit", [
    ("stage.3072", _set_len("p63", 1)),        # the last path one byte longer: range 3088
    ("stage.3073", _set_len("p63", -1)),
    ("gather.fit", _set_len("a0", 9)),         # 49 bytes: a 193rd chunk
    ("segcap.192/193", _slash_in("t192", 2)),  # a letter of the 192-entry group becomes a slash: 193 entries
    ("seg.64/65", _set_len("stay@1", 1)),      # the 64-byte segment takes the byte laid after it: 65
    ("fold.8/9", _slash_in("f8.0", 10)),       # the 8-segment path gains a ninth
    ("win.192/193", _set_len("w192.31", 1)),
    ("img.cap/over", _set_len("cap", 1)),
    ("slow.img4096", _set_len("long", -1)),
], ids=lambda x: x if isinstance(x, str) else "")
def test_census_fails_when_a_layout_moves_by_one_byte(name, edit):
    with pytest.raises(AssertionError):
        CENSUS[name](_perturbed(name, edit))


# ---------------------------------------------------------------------------
# the oracle against the Python restatement

@pytest.mark.parametrize("name", CPU_NAMES)
def test_oracle_equals_python_restatement(name):
    L = ul.layout(name)
    url_out, refs, arena, used = L.oracle({})
    py_out, py_tm = L.py_process()
    np.testing.assert_array_equal(url_out, py_out)
    lens = np.array([len(t) for t in py_tm], dtype=np.uint32)
    np.testing.assert_array_equal(np.where(url_out != 0, refs[:, 1], 0), lens)
    assert used == int(lens.sum())
    assert arena.tobytes() == b"".join(py_tm)          # span by span: the packed arena is the templates in span order
    np.testing.assert_array_equal(refs[url_out != 0, 0], (np.cumsum(lens) - lens)[url_out != 0])


def test_reference_name_equals_oracle_on_every_case():
    orc = UrlOracle({})
    n = 0
    for family, cases in ul.CASES.items():
        for label, seg, after in cases:
            for s in seg.split(b"/") + [seg.split(b"/")[-1] + after]:
                assert orc.segment_name(s) == ul.reference_name(s), (label, s)
                n += 1
    assert n > 300
    # the verdicts the cases are named for
    verdict = {label: ul.reference_name(seg) for cases in ul.CASES.values() for label, seg, _ in cases if b"/" not in seg}
    for L in (10, 11, 15, 16, 17, 19, 20, 21, 24):
        assert verdict[f"date.{L}"] == "date" and verdict[f"date.{L}+1"] != "date"
        assert (verdict[f"date.{L}-1"] == "date") == (L in (11, 17, 20))        # a zone "Z" less is a date again
    assert [k for k in verdict if k.startswith("date.") and ".p" in k and verdict[k] == "date"] == []
    assert [k for k in verdict if k.startswith("date.") and ".d" in k and verdict[k] == "date"] == []
    assert len([k for k in verdict if k.startswith("date.") and ".p" in k]) == 2 + 3 + 3 + 4 + 5 + 5 + 6 + 5 + 6
    assert verdict["date.zone3"] != "date" and verdict["date.zone5"] != "date"
    assert [verdict[f"hex.{n}"] for n in (14, 15, 16, 17, 18, 64)] == [None, None, "id", None, "id", "id"]
    assert verdict["hex.16g"] is None and verdict["hex.mixed"] == "id"
    assert verdict["digits.6"] is None and verdict["digits.7"] == "id" and verdict["digits.7end64"] == "id"
    assert verdict["digits.6end64"] is None
    assert [verdict[k] for k in ("uuid.36", "uuid.37pre", "uuid.37suf", "uuid.64end", "uuid.64start")] == ["id"] * 5
    assert verdict["uuid.mid"] is None and verdict["uuid.dash"] is None and verdict["uuid.35"] is None
    assert {k: v for k, v in verdict.items() if k.startswith("email.")} == {
        "email.at0": None, "email.two": None, "email.dot0": None, "email.dot1": "email", "email.tld1": None,
        "email.tld.digit": None, "email.pct": None, "email.64": "email", "email.local": "email"}
    assert verdict["noletters.empty"] is None and all(verdict[f"noletters.{k}"] == "id" for k in ("dash", "under", "pct", "one"))
    assert [k for k in verdict if k.startswith("fffd.") and verdict[k] is None] == ["fffd.v2", "fffd.v3", "fffd.v4", "fffd.e9"]


@pytest.mark.parametrize("name", CPU_NAMES)
def test_never_config_matches_nothing(name):
    # the config that selects url_plan_kernel<1>: its custom id and its rule match nothing on any layout
    L = ul.layout(name)
    a, b = L.oracle({}), L.oracle(ul.NEVER_CFG)
    assert a[3] == b[3]
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------
# GPU parity, bit for bit, with the witnesses

_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    """The engines the GPU tests of this module share (one per config) are released with the module."""
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()


def _engine(cfg, extra=None):
    from odigos_amd.batch import Engine
    key = repr((cfg, extra))
    if key not in _engines:
        full = {"odigosurltemplate": cfg}
        full.update(extra or {})
        eng = Engine(full)
        eng.set_option("url_path_counts", 1)
        _engines[key] = eng
    return _engines[key]


def _compare(L, db, cfg, refs):
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    url_out, orefs, oarena, oused = L.oracle(cfg)
    n = L.n
    np.testing.assert_array_equal(db.out_numpy("url_out")[:n], url_out)
    mask = url_out != 0
    used = db.used()
    gt = db.out_numpy("tmpl", np.uint32)[:2 * n]
    if not refs:
        np.testing.assert_array_equal(gt.reshape(-1, 2)[mask], orefs[mask])
        assert used == oused
        np.testing.assert_array_equal(db.out_numpy("tmpl_arena")[:used], oarena)
    else:
        cap = db.outs.tmpl_arena_cap
        # the gaps: <= 15 bytes per group and the waves' last chunk tails (<= cap / 8), as tests/test_url_refs.py states
        assert oused <= used <= min(cap, oused + 16 * L.n_groups + cap // 8)
        gb, gl = span_template_bytes(gt, db.out_numpy("tmpl_arena")[:used], mask)
        ob, ol = span_template_bytes(orefs.reshape(-1), oarena, mask)
        np.testing.assert_array_equal(gl, ol)
        np.testing.assert_array_equal(gb, ob)


def _gpu(L, cfg, refs, tmpl_cap=None):
    import torch
    from odigos_amd.batch import DeviceBatch
    eng = _engine(cfg)
    db = DeviceBatch(L.cols, tmpl_cap=tmpl_cap or ul.tmpl_cap(L))
    eng.process_device(db, native.STAGE_TEMPLATE | (REFS if refs else 0))
    torch.cuda.synchronize()
    _compare(L, db, cfg, refs)
    got = eng.path_counts()
    want = L.expect(cfg)
    assert got["url_unplanned"] == want["url_unplanned"]
    if L.n_groups <= K.kUrlMaxWaves:
        assert got["url_slow"] == want["url_slow"]


FORMS = {"default-packed": ({}, False), "default-refs": ({}, True), "general-packed": (ul.NEVER_CFG, False),
         "general-refs": (ul.NEVER_CFG, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SMALL)
def test_gpu_layout(name, form):
    cfg, refs = FORMS[form]
    _gpu(ul.layout(name), cfg, refs)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["default", "general"])
def test_gpu_refs_chunk_ends_at_an_image(cfg):
    # parity, and `used` within the bound tests/test_url_refs.py states (which chunk a wave gets depends on
    # the order of the waves' fetch-adds; what each span's ref names does not)
    _gpu(ul.layout("refs.chunk"), {} if cfg == "default" else ul.NEVER_CFG, True, tmpl_cap=ul.REFS_CHUNK_CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["packed", "refs"])
@pytest.mark.parametrize("name", list(ul.NAMES))
def test_gpu_names(name, form):
    L = ul.layout(name)
    _gpu(L, L.cfg, form == "refs")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default-packed", "general-packed"])
def test_gpu_dirty_then_seam(form):
    # one call per config: 2 x kUrlMaxWaves groups, so every plan wave takes a
    # seam group after a dirty one whatever the grid's stride
    cfg, refs = FORMS[form]
    _gpu(ul.layout(ul.DIRTY), cfg, refs)


def _with_size_columns(L):
    """The layout's columns with trivial odigostrafficmetrics columns: one
    resource, one scope, one attribute set."""
    n = L.n
    keep = dict(span_size=(100 + np.arange(n) % 7).astype(np.uint32), name_len=(3 + np.arange(n) % 5).astype(np.uint32),
                scope=np.zeros(n, dtype=np.uint32), resource=np.zeros(n, dtype=np.uint32),
                scope_size=np.array([10], dtype=np.uint32), scope_resource=np.zeros(1, dtype=np.uint32),
                res_size=np.array([20], dtype=np.uint32), res_attrset=np.zeros(1, dtype=np.uint32))
    c = native.Columns()
    C.memmove(C.byref(c), C.byref(L.cols), C.sizeof(c))
    c.n_resources = c.n_scopes = c.n_attrsets = 1
    for f, a in keep.items():
        setattr(c, f, a.ctypes.data)
    return c, keep


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["packed", "refs"])
@pytest.mark.parametrize("name", ["seg.64/65", "fold.8/9", "copy.tiny"])
def test_gpu_layout_with_size(name, form):
    # TEMPLATE | SIZE: the spans pass fused into url_copy_kernel<true, *> sees these template lengths
    import torch
    from odigos_amd.batch import DeviceBatch, HostOutputs
    L = ul.layout(name)
    cols, _keep = _with_size_columns(L)
    eng = _engine({}, {"odigostrafficmetrics": {"res_attributes_keys": ["service.name"]}})
    st = native.STAGE_TEMPLATE | native.STAGE_SIZE
    db = DeviceBatch(cols, tmpl_cap=ul.tmpl_cap(L))
    eng.process_device(db, st | (REFS if form == "refs" else 0))
    torch.cuda.synchronize()
    _compare(L, db, {}, form == "refs")
    ho = HostOutputs(cols, tmpl_cap=ul.tmpl_cap(L))
    assert UrlOracle({}).process(cols, ho.outs, 4) == 0
    assert size_process(cols, ho.outs, st, native.GROUP_TRACE_ID, ho.outs, 1, 1.0, 0.0, 4) == 0
    np.testing.assert_array_equal(db.out_numpy("attrset_bytes", np.int64)[:1], ho.view("attrset_bytes", np.int64)[:1])
    assert int(db.out_numpy("accepted_spans", np.int64)[0]) == int(ho.view("accepted_spans", np.int64)[0]) == L.n
    assert int(ho.view("attrset_bytes", np.int64)[0]) > 100 * L.n


@pytest.mark.gpu
def test_gpu_path_counts_option():
    from odigos_amd.batch import DeviceBatch, Engine
    import torch
    L = ul.layout("seg.64/65")
    eng = Engine({"odigosurltemplate": {}})
    with pytest.raises(native.OseError):
        eng.set_option("url_path_countz", 1)           # an unknown option is still OSE_EINVAL
    assert eng.L.ose_engine_set_option(eng.h, b"url_path_countz", 1) == native.OSE_EINVAL
    db = DeviceBatch(L.cols, tmpl_cap=ul.tmpl_cap(L))
    eng.process_device(db, native.STAGE_TEMPLATE)       # off by default: nothing is kept
    torch.cuda.synchronize()
    assert set(eng.path_counts()) == {"run_list", "sort", "long_runs"}
    cnt = (C.c_uint64 * 5)(7, 7, 7, 7, 7)
    assert eng.L.ose_engine_path_counts(eng.h, cnt, 5) == 5 and list(cnt) == [0, 0, 0, 0, 0]
    eng.set_option("url_path_counts", 1)
    eng.process_device(db, native.STAGE_TEMPLATE)
    c = eng.path_counts()
    assert (c["url_unplanned"], c["url_slow"]) == EXPECT["seg.64/65"] and (c["run_list"], c["sort"], c["long_runs"]) == (0, 0, 0)
    cnt = (C.c_uint64 * 5)(7, 7, 7, 7, 7)
    assert eng.L.ose_engine_path_counts(eng.h, cnt, 3) == 5      # cap bounds the write, not the count
    assert list(cnt) == [0, 0, 0, 7, 7]
    eng.set_option("url_path_counts", 0)                          # off again: the words keep the last call they saw
    eng.process_device(DeviceBatch(ul.layout("gates").cols), native.STAGE_TEMPLATE)
    c = eng.path_counts()
    assert (c["url_unplanned"], c["url_slow"]) == EXPECT["seg.64/65"]
    eng.close()
