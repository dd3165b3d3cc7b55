"""Source check: every kernel launch in gs_engine.cpp takes the x dimension
of its grid from grid_for or grid_items, the two helpers that the debug cap
(gs_debug_set_grid_cap) acts on.  A launch with a hand-written cap would
escape the grid-stride tests of test_gpu_grid_stride.py, so it fails here
until it is routed through a helper or listed as exempt, with a reason."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "cnosdb_amd", "csrc", "gs_engine.cpp")
HDR = os.path.join(REPO, "include", "cnosdb_gs.h")

# kernel -> the exact grid it is allowed to keep, and why
EXEMPT = {
    # the grid IS the work split of the two-level scan (one partial per
    # block, at most 2048 of them for k_scan_fixup's single pass): more
    # groups are refused, not strided over
    "k_scan_partials": "dim3(nblocks)",
    # one wave sums the block totals
    "k_scan_fixup": "dim3(1)",
    # repro tooling, fixed 64 blocks
    "k_debug_crc": "dim3(64)",
}
# variables that may stand for a helper's result at a launch; every
# assignment to them in the file must come from a helper
GRID_VARS = ("blocks", "pl.gx")
HELPER = re.compile(r"^grid_(for|items)\(.*\)$", re.S)


def _args(src, pos):
    """Top-level arguments of the call whose '(' is at src[pos]."""
    assert src[pos] == "("
    depth, start, out = 0, pos + 1, []
    for i in range(pos, len(src)):
        c = src[i]
        if c == "(":
            depth += 1
        elif c == ")":
            depth -= 1
            if depth == 0:
                out.append(src[start:i])
                return out
        elif c == "," and depth == 1:
            out.append(src[start:i])
            start = i + 1
    raise AssertionError("unbalanced call")


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def launches(src):
    """(kernel, normalised grid argument, line) of every launch."""
    out = []
    for m in re.finditer(r"hipLaunchKernelGGL\s*\(", src):
        a = _args(src, m.end() - 1)
        kern = re.sub(r"<.*>", "", _norm(a[0]))
        out.append((kern, _norm(a[1]), src.count("\n", 0, m.start()) + 1))
    return out


def grid_x(grid):
    """First component of a dim3(...) grid argument."""
    m = re.match(r"^dim3\s*\(", grid)
    assert m, grid
    return _norm(_args(grid, m.end() - 1)[0])


def bad_sites(src):
    bad = []
    for kern, grid, line in launches(src):
        if kern in EXEMPT:
            if grid != EXEMPT[kern]:
                bad.append((kern, grid, line))
            continue
        x = grid_x(grid)
        if HELPER.match(x):
            continue
        if x in GRID_VARS:
            continue
        bad.append((kern, grid, line))
    return bad


def test_every_launch_takes_its_grid_from_a_helper():
    src = open(SRC).read()
    sites = launches(src)
    assert len(sites) >= 50, len(sites)  # the parser sees the launches
    assert not bad_sites(src), bad_sites(src)
    # each exempt launch still exists: a stale allow-list entry is removed
    kernels = {k for k, _, _ in sites}
    assert set(EXEMPT) <= kernels, set(EXEMPT) - kernels


def test_grid_variables_are_only_assigned_from_a_helper():
    src = open(SRC).read()
    for var in GRID_VARS:
        pat = re.compile(r"(?<![\w.])" + re.escape(var) +
                         r"\s*=(?!=)\s*([^;]*);")
        rhs = [_norm(m.group(1)) for m in pat.finditer(src)]
        assert rhs, var
        for r in rhs:
            assert HELPER.match(r), (var, r)


def test_no_hand_written_cap_is_left():
    """The only comparisons with the old caps are the functional limit of the
    two-level scan."""
    src = open(SRC).read()
    lines = [l.strip() for l in src.splitlines()
             if re.search(r">\s*(2048|65535)\b", l)]
    assert lines and all(l == "if (nblocks > 2048)" for l in lines), lines


def test_the_check_catches_a_hand_written_cap():
    bad = ("void f() { hipLaunchKernelGGL(k_new, dim3(n > 2048 ? 2048 : n),"
           " dim3(256), 0, s, a, b); }")
    assert [k for k, _, _ in bad_sites(bad)] == ["k_new"]
    moved = "hipLaunchKernelGGL(k_scan_fixup, dim3(2), dim3(64), 0, s, a);"
    assert [k for k, _, _ in bad_sites(moved)] == ["k_scan_fixup"]
    good = ("hipLaunchKernelGGL(k_new<true>, dim3(grid_items(n, 2048), ny),"
            " dim3(256), 0, s, a);")
    assert not bad_sites(good)


def test_seam_is_not_public_and_reads_no_environment():
    assert "gs_debug_" not in open(HDR).read()
    src = open(SRC).read()
    m = re.search(r"static int grid_items\(.*?\n}\n", src, re.S)
    assert m and "getenv" not in m.group(0)
    assert re.search(r"static std::atomic<int> g_grid_cap\b", src)
