"""The cell rules of gs_agg_group (cnosdb_amd/csrc/gs_agg.h), run on the
host: the header the aggregate kernels and the entry point share also
compiles as plain C++, so agg_add_row, agg_combine and the bucket index are
exercised by a stand-alone program (tests/cpu/agg_check.cpp) under
AddressSanitizer and UBSan: every cell of the hand-written table and 300
random runs of at most 40 rows, folded row by row and in every split into 2
and 3 pieces, and the bucket index at the int64 extremes.  Expectations are
agg_ref's."""
import pytest

import agg_ref as ar
import filter_ref as fr


def test_runs_and_probes_cover_the_rules():
    runs = ar.hand_runs() + ar.random_runs()
    assert len(ar.random_runs()) >= 300
    assert max(len(rows) for _, rows in runs) == 40
    assert any(len(rows) == 0 for _, rows in runs)
    assert {ct for ct, _ in runs} == {fr.CT_I64, fr.CT_F64, fr.CT_BOOL,
                                      fr.CT_U64}
    # equal timestamps inside a run, and null cells
    assert any(a[0] == b[0] for _, rows in runs
               for a, b in zip(rows, rows[1:]))
    assert any(not v for _, rows in runs for _, _, _, v in rows)
    probes = ar.bucket_probes()
    ends = {(ts, t0) for ts, t0, _, _ in probes}
    assert (fr.I64_MIN, fr.I64_MAX) in ends and (fr.I64_MAX, fr.I64_MIN) in ends
    widths = {bn for _, t0, bn, _ in probes if abs(t0) == fr.I64_MAX
              or t0 == fr.I64_MIN}
    assert {1, fr.I64_MAX} <= widths


def test_agg_rules_host_sanitized(tmp_path):
    """No case is skipped or filtered: the program's summary carries the
    number of runs and probes written."""
    run = ar.run_host_check(tmp_path, sanitize=True)
    if run is None:
        pytest.skip("no host C++ compiler")
    res, nruns, nprobes = run
    assert nruns == len(ar.hand_runs()) + 300 and nprobes > 100
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stderr == ""  # the sanitizers stay silent
    assert f"{nruns} runs, " in res.stdout
    assert f" {nprobes} probes, " in res.stdout
    assert res.stdout.rstrip().endswith(" 0 failures")
