"""The definition of a row list (tests/row_lists.py) checked against what it is for -- no GPU.

  * dropping is exact: per centre, the listed rows are the same SET of (source point, relative coordinates bit for bit) as all nsample
    slots of the index row -- why the packed kernels pool the same bits as the unpacked one;
  * the counts are the formulas of test_gpu_shadow.check_ball_pack (the header check of the whole-engine run), reused from there;
  * the generators planted the edge cases the kernels' branches need;
  * every clause of the definition is exercised by the inputs: a one-line mutant of it gives a different list."""
import collections
import types

import numpy as np
import pytest
import torch

import row_lists as R
from test_gpu_shadow import check_ball_pack

CASES = R.ONE_WORKGROUP + R.TWO_LAUNCH


def _sources(k, case, i):
    """the distinct point behind point k of cloud i: k % lim, then its representative"""
    k = np.asarray(k, np.int64)
    if case.limit is not None:
        k = k % max(int(case.limit[i]), 1)
    if case.rep is not None:
        k = case.rep[i].astype(np.int64)[k]
    return k


def _row_set(centre, source, dxyz):
    return np.unique(np.concatenate([centre[:, None], source[:, None], dxyz[:, :3].view(np.uint32).astype(np.int64)], 1), axis=0)


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_dropping_rows_is_exact(c):
    case, clouds = R.case(*c)
    b, m, ns = case.idx.shape
    for i in range(b):
        idx = case.idx[i].astype(np.int64)
        centre = np.repeat(np.arange(m), ns)
        d_all = np.ascontiguousarray(case.xyz[i][idx.reshape(-1)] - case.new_xyz[i][centre])
        own = np.ones(m, bool) if case.crep is None else case.crep[i] == np.arange(m)
        sel = own[centre]
        every_slot = _row_set(centre[sel], _sources(idx.reshape(-1), case, i)[sel], d_all[sel])
        info, dxyz, cnt = clouds[i]
        listed = _row_set((info >> 16).astype(np.int64), _sources(info & 0xffff, case, i), np.ascontiguousarray(dxyz))
        assert np.array_equal(every_slot, listed), (c, i)
        assert (dxyz[:, 3] == 0).all() and np.array_equal(np.bincount((info >> 16).astype(np.int64), minlength=m), cnt)
        if case.crep is not None:      # a copy centre is its representative over again: its slots are the representative's slots
            r = case.crep[i]
            assert np.array_equal(case.idx[i], case.idx[i][r]) and np.array_equal(case.new_xyz[i].view(np.uint32), case.new_xyz[i][r].view(np.uint32))
            assert (cnt[~own] == 0).all()


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_counts_equal_the_formulas_of_the_engine_shadow(c):
    case, clouds = R.case(*c)
    info, dxyz, tilecloud, (tiles, rows) = R.packed_list(clouds)
    t = lambda a: None if a is None else torch.from_numpy(a)
    pack = types.SimpleNamespace(hdr=torch.tensor([tiles, rows, 0, 0], dtype=torch.int32), tilecloud=torch.from_numpy(tilecloud))
    shadow = types.SimpleNamespace(_log=collections.Counter())
    check_ball_pack(shadow, R.case_id(c), None, [t(case.idx), t(case.xyz), t(case.new_xyz), t(case.limit), t(case.rep), t(case.crep)], pack)
    assert len(info) == tiles * R.ROWS == len(dxyz) and tiles == sum((len(cl[0]) + R.ROWS - 1) // R.ROWS for cl in clouds)
    if case.rep is not None:
        assert shadow._log["rep_rows_dropped"] > 0
    if case.crep is not None:
        assert shadow._log["centres_skipped"] > 0


WANT_PLANTED = {
    "plain": {"full_row", "cnt_one", "total_multiple_of_64", "total_not_multiple_of_64", "fewer_than_64_rows", "tile_starts_on_a_chunk_boundary",
              "tile_straddles_a_chunk_boundary", "short_last_chunk_with_rows", "padding_is_not_the_last_row"},
    "arbitrary": {"full_row", "cnt_one", "padding_is_not_the_last_row"},
}
WANT_PLANTED["limit"] = WANT_PLANTED["plain"] | {"slot_beyond_limit_inside_the_prefix", "limit_zero_and_one", "copies_listed_after_originals"}
WANT_PLANTED["rep"] = WANT_PLANTED["plain"] | {"copy_before_a_kept_slot"}
WANT_PLANTED["crep"] = WANT_PLANTED["plain"] | {"last_centre_is_a_copy", "last_centre_owns_rows", "empty_chunk_in_the_middle", "empty_last_chunk"}
WANT_PLANTED["rep+crep"] = (WANT_PLANTED["rep"] | WANT_PLANTED["crep"]) - {"empty_chunk_in_the_middle", "empty_last_chunk"}   # (rep: never two launches)
WANT_PLANTED["limit+crep"] = WANT_PLANTED["limit"] | WANT_PLANTED["crep"]
WANT_PLANTED["limit+rep"] = WANT_PLANTED["limit"] | WANT_PLANTED["rep"]


@pytest.mark.parametrize("form", R.FORMS)
def test_planted_edge_cases_are_present(form):
    """make_case asserts each edge case it plants; here: every case of the form planted what its size allows, and the form's cases
    together hold every edge case the form has"""
    seen = set()
    for c in CASES:
        if c[0] != form:
            continue
        planted = R.case(*c)[0].planted
        assert planted and all(planted.values()), (c, planted)
        seen |= set(planted)
        if c[2] >= R.TWO_LAUNCH_M:      # the two-launch kernels: everything about chunks, in every single case
            assert {"tile_starts_on_a_chunk_boundary", "tile_straddles_a_chunk_boundary", "total_multiple_of_64"} <= set(planted), c
            if "crep" in form:
                assert {"empty_chunk_in_the_middle", "empty_last_chunk", "last_centre_is_a_copy", "fewer_than_64_rows"} <= set(planted), c
    assert seen == WANT_PLANTED[form], (form, seen ^ WANT_PLANTED[form])
    ms = {c[2] for c in CASES if c[0] == form}
    assert ms >= {37, 511} and (form not in ("plain", "limit", "crep", "limit+crep") or ms >= {512, 600, 1024})


def _applies(mutant, form):
    # (limit together with rep: a point k >= lim is a copy of k % lim, so a map that names the LOWEST copy has rep[k] < lim <= k and the
    #  mask drops the slot whether `< lim` is asked or not -- the clause cannot show there)
    return {"pad_with_last_row": True, "ignore_limit": "limit" in form and "rep" not in form.split("+"), "rep_as_prefix": "rep" in form.split("+"),
            "ignore_crep": "crep" in form}[mutant]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_clause_of_the_definition_is_exercised(mutant):
    """a clause that no input exercises would let a producer get it wrong unnoticed: in EVERY case whose form has the clause, the
    definition with that clause changed lists something else"""
    n = 0
    for c in CASES:
        if not _applies(mutant, c[0]):
            continue
        case, clouds = R.case(*c)
        other = R.row_list(case.idx, case.xyz, case.new_xyz, case.limit, case.rep, case.crep, _mutant=mutant)
        a, o = R.packed_list(clouds), R.packed_list(other)
        same = a[3] == o[3] and np.array_equal(a[0], o[0]) and np.array_equal(a[1].view(np.uint32), o[1].view(np.uint32))
        assert not same, (mutant, c)
        n += 1
    assert n >= 6          # (rep never meets the two-launch kernels: its three forms at two sizes)
