"""The material sort's cases (tests/sort_cases.py) from the oracle alone, no device: what tests/test_gpu_sort_keys.py compares
the three device forms with cannot be vacuous.

First the oracle's own order is held against an independent statement of it -- the pool after a bounce is the stable sort of the
entering pool by key, then the stable partition by survival (sort_cases.expected_order) -- and its path states against the
unsorted oracle's.  Then the coverage floors: what the rooms put in front of the kernels, per 64-path tile, per 128-path strip
(one wave's share of a chunk) and per 512-path chunk of the pool that enters a bounce.  Floors are conditions on the room, not
measurements of the code under test; the value measured on the room as it stands is written beside each.

Three cases cannot meet two of the floors stated for `every compacting case`, by their own definition: in f1, w1 and g65e every
hit ends the path, so their live counts are [3072, 0, ...] (a floor of its own below) -- both multiples of 64 and of 512 -- and
their only ties are between paths that end.  For them the tie check reads the whole sorted pool of bounce 0 (the oracle's snapshot
keeps the ended paths behind the live ones, in sorted order) and the ragged-count floor is not asked.

The refusals of pt_init (65 materials with the flags that need the fused form, 2048 materials) come after its device check, so
they live in the GPU module."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import sort_cases as sc  # noqa: E402

COMPACTING = [r for r in sc.RUNS if sc.BY_ID[r[0]].compact]
ENDS_AT_ONCE = ("f1", "w1", "g65e")                                  # every hit ends the path
ITS = (1, 2)


@pytest.fixture(scope="module")
def pt():
    p = ge.load_package()
    p.build_host()
    return p


def pools(po, pt, run):
    """[(it, d, keys entering bounce d, pixel indices entering it)] over two iterations, bounces with a non-empty pool."""
    def make():
        case = sc.BY_ID[run[0]]
        ref = sc.reference(po, pt, case, run[1])
        geoms, _ = sc.scene_of(pt, case)
        out = []
        for it in ITS:
            for d in range(len(ref.snaps[it])):
                pool = sc.entering(po, ref, run[1], it, d)
                if len(pool):
                    out.append((it, d, sc.keys_entering(po, geoms, case.M, pool), pool["pixelIndex"].copy()))
        return out
    key = ("pools",) + run
    if key not in sc._cache:
        sc._cache[key] = make()
    return sc._cache[key]


def test_the_table_is_the_hosts_rule():
    """Every case names the form that pt_init's and enqueue_bounce's rule gives its material count and flags, every form has
    cases on both sides of its limits, and ids are unique."""
    assert len({c.id for c in sc.CASES}) == len(sc.CASES)
    for c in sc.CASES:
        assert sc.form_of(c) == c.form, c.id
    forms = {c.id: c.form for c in sc.CASES}
    assert forms["f64"] == "fused" and forms["g65"] == "workgroup"               # M = 64 -> 65 without PT_UNFUSED
    assert forms["w63"] == "wave" and forms["g64"] == "workgroup"                # 64 -> 65 bins with it
    assert forms["n63"] == "wave" and forms["n65"] == "workgroup"
    assert sc.BY_ID["g2047"].nbins == sc.SORT_MAX_BINS
    assert (sc.BY_ID["g127"].nbins + 3) & ~3 == 128 and (sc.BY_ID["g128"].nbins + 3) & ~3 == 132


def test_the_room(pt):
    """145 primitives, every key used up to M = 145, keys near M - 1 beyond; M = 1 and all_emissive are rooms of emitters."""
    for M in (1, 2, 63, 64, 65, 128, 145, 2047):
        geoms, mats = sc.mosaic_room(pt, M)
        assert len(geoms) == sc.N_GEOMS == 145 and len(mats) == M
        used = np.unique(geoms["materialid"])
        assert used.min() == 0 and used.max() == M - 1
        if M <= 145:
            assert len(used) == M
        assert np.isfinite(geoms["inverseTransform"]).all() and (geoms["rotation"] == 0).all()
        kind = np.arange(M) % 8
        assert ((mats["emittance"] > 0) == (kind == sc.EMITTER)).all()
        assert ((mats["hasReflective"] > 0) == (kind == sc.MIRROR)).all() and ((mats["hasRefractive"] > 0) == (kind == sc.GLASS)).all()
    assert (sc.mosaic_room(pt, 65, all_emissive=True)[1]["emittance"] > 0).all()
    a, b = sc.mosaic_room(pt, 65), sc.mosaic_room(pt, 65)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("run", COMPACTING, ids=sc.run_id)
def test_oracle_order_is_the_specification(po, pt, run):
    """After every bounce the oracle's live prefix is expected_order of the keys that entered, the ended paths behind it are the
    rest in the same order, and the path states are the unsorted oracle's for the same pixels, bit for bit."""
    case = sc.BY_ID[run[0]]
    ref, plain = sc.reference(po, pt, case, run[1]), sc.unsorted_reference(po, pt, case, run[1])
    geoms, _ = sc.scene_of(pt, case)
    for it in ITS:
        assert ref.live[it] == plain.live[it] and ref.rays[it] == plain.rays[it]
        assert ref.images[it].tobytes() == plain.images[it].tobytes()
        assert len(ref.snaps[it]) == len(plain.snaps[it])
        for d, (s, u) in enumerate(zip(ref.snaps[it], plain.snaps[it])):
            pool = sc.entering(po, ref, run[1], it, d)
            assert len(pool) == s["n_before"]
            keys = sc.keys_entering(po, geoms, case.M, pool)
            after = s["paths"]
            live = after["pixelIndex"][:s["n_live"]]
            ended = after["pixelIndex"][s["n_live"]:]
            assert (after["remainingBounces"][:s["n_live"]] > 0).all() and (after["remainingBounces"][s["n_live"]:] <= 0).all()
            assert np.array_equal(live, sc.expected_order(keys, pool["pixelIndex"], live)), (run, it, d)
            assert np.array_equal(ended, sc.expected_order(keys, pool["pixelIndex"], ended)), (run, it, d)
            assert len(np.unique(live)) == len(live)
            # the same paths, whatever the order: shading does not depend on where a path sits in the pool
            assert s["n_live"] == u["n_live"]
            a = after[:s["n_live"]][np.argsort(live, kind="stable")]
            b = u["paths"][:u["n_live"]]
            b = b[np.argsort(b["pixelIndex"], kind="stable")]
            assert a.tobytes() == b.tobytes(), (run, it, d)


def reversed_ties(keys, pixel_index, survivors):
    """expected_order with equal keys in reverse: what an unstable sort could give."""
    idx = np.lexsort((-np.arange(len(keys)), keys))
    order = np.asarray(pixel_index)[idx]
    return order[np.isin(order, survivors)]


@pytest.mark.parametrize("run", COMPACTING, ids=sc.run_id)
def test_an_unstable_sort_would_show(po, pt, run):
    """>= 10 pairs of equal keys inside one tile at some bounce, and reversing the ties changes the pool the oracle leaves."""
    case = sc.BY_ID[run[0]]
    ref = sc.reference(po, pt, case, run[1])
    ps = pools(po, pt, run)
    # measured: 2016 in every case -- a tile of bounce 0 that misses, or hits the one emitter, as a whole; the least over the later
    # bounces is 186 .. 421 at 64 x 48 and 128 x 72
    assert max(sc.same_key_pairs_in_a_tile(keys) for _, _, keys, _ in ps) >= 10
    differs = 0
    for it, d, keys, pix in ps:
        s = ref.snaps[it][d]
        after = s["paths"]["pixelIndex"]
        want = after[:s["n_live"]] if case.id not in ENDS_AT_ONCE else after
        assert np.array_equal(want, sc.expected_order(keys, pix, want))
        differs += not np.array_equal(want, reversed_ties(keys, pix, want))
    assert differs >= 1                  # measured: most bounces of every case; 6 of the 12 at 67 x 5 (pools of 2 to 13 paths)


@pytest.mark.parametrize("run", COMPACTING, ids=sc.run_id)
def test_coverage_floors(po, pt, run):
    case, (w, h) = sc.BY_ID[run[0]], run[1]
    ref = sc.reference(po, pt, case, run[1])
    _, mats = sc.scene_of(pt, case)
    ps = pools(po, pt, run)
    M = case.M
    emits = np.append(mats["emittance"] > 0, False)                  # per key; the miss bin is no material
    tile = max(sc.distinct_in_runs(keys, sc.TILE) for _, _, keys, _ in ps)
    strip = max(sc.distinct_in_runs(keys, sc.STRIP) for _, _, keys, _ in ps)
    chunk = max(sc.distinct_in_runs(keys, sc.CHUNK) for _, _, keys, _ in ps)
    populated = lambda k: any((keys == k).any() for _, _, keys, _ in ps)          # noqa: E731
    live = [n for it in ITS for n in ref.live[it]]
    big = M >= 63 and w * h >= 64 * 48 and not case.all_emissive
    if big:
        # measured at some bounce -- tile: 37 .. 47, strip: 50 .. 74, chunk: 64 .. 136 (M = 62, below the condition: 39, 50, 63)
        assert tile >= 24 and strip >= 40 and chunk >= 60, (tile, strip, chunk)
        assert populated(0) and populated(M - 1) and populated(M)    # measured at bounce 0: 17 .. 87, 1 .. 19 and 1051 (4731) paths
        for it, d, keys, _ in ps:
            present = np.unique(keys)
            # measured: 7 .. 19 emitter keys beside 52 .. 126 surviving ones at every bounce
            assert emits[present].any() and (~emits[present[present < M]]).any(), (it, d)
    if case.id == "g65" and (w, h) != sc.FRAME:
        assert populated(0) and populated(M - 1) and populated(M)    # measured: 1, 1, 319 at bounce 0 (67 x 5); 3, 0, 1098 there and 13, 3 over the bounces (130 x 9)
        assert (w * h) % sc.TILE and (w * h) % sc.CHUNK              # a partly filled tile and chunk: 335 = 5 x 64 + 15, 1170 = 2 x 512 + 146
    if M >= 127:
        assert strip >= 56 and chunk >= 100, (strip, chunk)          # measured: strip 68 .. 74, chunk 122 .. 136
    if case.id not in ENDS_AT_ONCE:
        # measured: no live count after bounce 0 is a multiple of 64 in any case (1083, 1817, 1812, 1652, 13, 57, 1864, 3998, ...)
        assert any(n % sc.TILE for n in live) and any(n % sc.CHUNK for n in live), live
    else:
        assert ref.live[1] == [w * h, 0, 0, 0, 0, 0] == ref.live[2]
        assert len(ref.snaps[1]) == 1                                # the oracle stops; the device still launches bounces 1 .. 5 on nothing
    nbins = case.nbins
    if run == ("g2047", (128, 72)):
        assert nbins * -(-w * h // sc.CHUNK) == 2048 * 18 > 32768    # the scan's stepped path
    if run == ("g2047", sc.FRAME):
        assert nbins * -(-w * h // sc.CHUNK) == 2048 * 6 <= 32768    # its one-barrier path, at the largest table that takes it here
    if case.id == "g64":
        assert nbins * -(-w * h // sc.CHUNK) == 65 * 6 and (65 * 6) % 4 != 0      # ... and its ragged tail
    if case.id == "g65":                                             # the ENV branch of the shading variants: misses per bounce
        if (w, h) == sc.FRAME:
            for it in ITS:
                for d in range(3):
                    keys = [k for i, dd, k, _ in ps if (i, dd) == (it, d)][0]
                    assert (keys == M).sum() >= 100                  # measured: 1051, 434 .. 437, 227 .. 238


def test_uncompacted_cases_share_the_rooms(pt):
    """n63 and n65 run on f63's / w63's and g65's rooms (the room depends on M alone): the floors above are theirs."""
    for a, b in (("n63", "w63"), ("n63", "f63"), ("n65", "g65")):
        ga, ma = sc.scene_of(pt, sc.BY_ID[a])
        gb, mb = sc.scene_of(pt, sc.BY_ID[b])
        assert ga.tobytes() == gb.tobytes() and ma.tobytes() == mb.tobytes()
