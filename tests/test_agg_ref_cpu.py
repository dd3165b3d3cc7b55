"""tests/agg_ref.py held to its hand-written table, and the conditions on
the designed and fuzzed cases that the device tests rely on.  No device, no
compiled code: the reference alone."""
import math

import numpy as np

import agg_ref as ar
import filter_ref as fr


def test_agg_ref_gives_the_hand_written_cells():
    assert len(ar.HAND) >= 13
    for h in ar.HAND:
        assert len(h.ac.case.ts) <= 12, h.name  # a person can check it
        bad = ar.check_against_hand(h, ar.agg_ref(h.ac))
        assert not bad, bad


def test_hand_table_covers_the_rules():
    """Each rule of the contract is met by some row or cell of the table."""
    seen = set()
    for h in ar.HAND:
        ac, case = h.ac, h.ac.case
        col = case.cols[0]
        ts = np.asarray(case.ts, np.int64)
        keep = fr.filter_ref(case).keep
        if col.valid is not None and (keep & ~np.asarray(col.valid)).any():
            seen.add("null cell")
        if col.tombs and (keep & fr.in_ranges(ts, col.tombs)).any():
            seen.add("column tombstone")
        if case.row_tombs and fr.in_ranges(ts, case.row_tombs).any():
            seen.add("row tombstone")
        buckets = [ar.bucket_of(t, ac.t0, ac.bucket_ns, ac.n_buckets)
                   for t in ts]
        if case.time_range and any(
                b is not None and not (case.time_range[0] <= t
                                       <= case.time_range[1])
                for t, b in zip(ts, buckets)):
            seen.add("range edge inside a bucket")
        if ac.bucket_ns and (ts[keep] < ac.t0).any():
            seen.add("ts < t0")
        if ac.bucket_ns and any(
                k and (int(t) - ac.t0) // ac.bucket_ns == ac.n_buckets
                for t, k in zip(ts, keep) if t >= ac.t0):
            seen.add("ts in bucket n_buckets")
        if ac.bucket_ns == 0:
            seen.add("bucket_ns 0")
        if col.ctype == fr.CT_F64:
            v = np.asarray(col.val, np.float64)
            if np.isnan(v).any():
                seen.add("NaN")
            z = v[v == 0]
            if z.size >= 2 and np.signbit(z).any() and not np.signbit(z).all():
                seen.add("zeros, first " + ("-" if np.signbit(z[0]) else "+"))
        if col.ctype == fr.CT_I64:
            total = sum(int(x) for x in col.val)
            if not fr.I64_MIN <= total <= fr.I64_MAX:
                seen.add("i64 sum wraps")
        if col.ctype == fr.CT_U64 and any(int(x) > 2**63 for x in col.val):
            seen.add("u64 above 2^63")
        if col.ctype == fr.CT_BOOL:
            seen.add("bool")
        if 0 in h.want["rows"]:
            seen.add("empty cell")
        if not ac.per_series and len(case.sizes) > 1:
            first = min(ts)
            if list(ts).count(first) > 1:
                seen.add("tie across series")
    want = {"null cell", "column tombstone", "row tombstone",
            "range edge inside a bucket", "ts < t0", "ts in bucket n_buckets",
            "bucket_ns 0", "NaN", "zeros, first +", "zeros, first -",
            "i64 sum wraps", "u64 above 2^63", "bool", "empty cell",
            "tie across series"}
    assert want <= seen, want - seen
    # every empty-cell convention is written down at least once
    empties = {h.ac.case.cols[0].ctype for h in ar.HAND if 0 in h.want["rows"]}
    assert empties == {fr.CT_I64, fr.CT_F64, fr.CT_U64, fr.CT_BOOL}


def test_bucket_rule_at_the_int64_ends():
    assert ar.bucket_of(fr.I64_MAX, fr.I64_MIN, 1, 4) is None
    assert ar.bucket_of(fr.I64_MIN, fr.I64_MAX, 1, 4) is None
    assert ar.bucket_of(fr.I64_MAX, fr.I64_MIN, fr.I64_MAX, 3) == 2
    assert ar.bucket_of(fr.I64_MAX, fr.I64_MAX, fr.I64_MAX, 1) == 0
    assert ar.bucket_of(5, 100, 0, 1) == 0
    probes = ar.bucket_probes()
    assert any(ts - t0 > fr.I64_MAX for ts, t0, _, _ in probes)


def test_sum_rule():
    b = lambda v: fr.bits(fr.CT_F64, v)  # noqa: E731
    assert ar.sum_within(fr.CT_F64, b(0.1 + 0.2), b(0.30000000000000004), 2,
                         0.30000000000000004)
    assert not ar.sum_within(fr.CT_F64, b(1.0 + 2.0**-40), b(1.0), 2, 1.0)
    assert ar.sum_within(fr.CT_F64, b(fr.NAN), b(fr.NAN), 3, 1.0)
    assert not ar.sum_within(fr.CT_F64, b(1.0), b(fr.NAN), 3, 1.0)
    assert ar.sum_within(fr.CT_F64, b(-0.0), b(0.0), 1, 0.0)
    assert not ar.sum_within(fr.CT_I64, 5, 6, 2, 0.0)


def test_fuzz_corpus_is_conditioned():
    """At least three quarters of the 50 cases have two non-empty and one
    empty cell, and keep some rows but not all; every type and every
    aggregate occurs; both cell layouts occur."""
    cases = [ar.fuzz_case(s) for s in ar.FUZZ_SEEDS]
    assert len(cases) == 50
    good_cells = good_keep = 0
    types, names, layouts = set(), set(), set()
    for ac in cases:
        assert len(ac.case.ts) <= 20000
        ref = ar.agg_ref(ac)
        nonempty = sum(1 for n in ref["rows"] if n)
        if nonempty >= 2 and nonempty < len(ref["rows"]):
            good_cells += 1
        kept = int(fr.filter_ref(ac.case).keep.sum())
        if 0 < kept < len(ac.case.ts):
            good_keep += 1
        for col, want in ac.aggs:
            types.add(ac.case.cols[col].ctype)
            names.update(want)
        layouts.add(ac.per_series)
    assert good_cells * 4 >= 3 * len(cases), good_cells
    assert good_keep * 4 >= 3 * len(cases), good_keep
    assert types == {fr.CT_I64, fr.CT_F64, fr.CT_BOOL, fr.CT_U64}
    assert names == set(ar.NAMES)
    assert layouts == {True, False}
    # the f64 sums of the corpus exercise the tolerance: some cell sums more
    # than one finite value
    assert any(c > 1 and math.isfinite(ar.value_of(fr.CT_F64, s))
               for ac in cases
               for (col, _), res in zip(ac.aggs, ar.agg_ref(ac)["cols"])
               if ac.case.cols[col].ctype == fr.CT_F64
               for c, s in zip(res["count"], res["sum"]))
