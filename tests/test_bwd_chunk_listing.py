"""CPU tier: where the wide build's backward sweep keeps its registers, read from the ISA hipcc generates (no GPU needed). The
Jacobian lanes of a chunk are inlined into backward_sweep so that the register save of a function that uses every VGPR is paid
once per sweep, in backward_sweep's prologue and epilogue, and not once per chunk — which holds only while the allocator keeps
everything inside the chunk loop in registers. Checked here with the project's own listing tools (tools/resource_usage.py,
tools/isa_stats.py): no scratch instruction inside the chunk loop of any backward_sweep of the wide unit (the three tangent loops
lie inside it), none in any function called from that loop, none in riccati_rows, no spilled VGPR in the wide kernels."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats  # noqa: E402
import resource_usage as ru  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """(listing path, compiler remarks, demangled names) of the wide unit, compiled once"""
    s, err = ru.compile_unit("tsat_kernels.hip", str(tmp_path_factory.mktemp("wide")))
    return s, ru.kernel_remarks(err), ru.function_info(s)


def bodies(path):
    """per function of a listing: its lines in order, labels (`name:`) and instructions, comments and directives aside"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "BB")):
            cur = out.setdefault(m.group(1), [])
            continue
        t = re.sub(r";.*$", "", line).strip()
        if cur is not None and t and (not t.startswith(".") or t.endswith(":")):
            cur.append(t)
    return out


def loops(body):
    """(first, last) line index of every loop: a branch to a label above it"""
    lab = {t[:-1]: i for i, t in enumerate(body) if t.endswith(":")}
    return [(lab[t.split()[-1]], i) for i, t in enumerate(body)
            if t.startswith(("s_cbranch", "s_branch")) and lab.get(t.split()[-1], i) < i]


def chunk_loop(body):
    """the outermost loop of a backward_sweep that calls riccati_rows"""
    with_call = [(a, b) for a, b in loops(body) if any("riccati_rows" in t and "@rel32" in t for t in body[a:b])]
    assert with_call, "no loop around the call of riccati_rows"
    return min(with_call, key=lambda ab: (ab[0], -ab[1]))


def test_no_scratch_inside_the_chunk_loop_of_the_wide_backward_sweep(wide):
    s, _, info = wide
    fb = bodies(s)
    sweeps = [n for n in fb if "backward_sweep" in n]
    assert len(sweeps) == 12                                     # rk3 / rk4 x three inertia classes x full / error state
    assert not [n for n in fb if "jacobian_chunk" in n and "tv_" not in n], "jacobian_chunk is inlined in the wide unit"
    for n in sweeps:
        a, b = chunk_loop(fb[n])
        # the tangent loops are 179 .. 527 instructions long, variant by variant; the only other loop inside the chunk loop, the
        # path of the lanes beyond the chunk's knots round the call of riccati_rows, is under 40: 100 tells them apart
        inner = [ab for ab in loops(fb[n]) if a < ab[0] and ab[1] < b and ab[1] - ab[0] > 100]
        assert len(inner) >= 3, (n, "the three tangent loops lie inside the chunk loop")
        assert not [t for t in fb[n][a:b + 1] if t.startswith("scratch_")], n
        for callee in {m.group(1) for t in fb[n][a:b + 1] for m in [re.search(r"(_Z\w+)@rel32", t)] if m}:
            assert info[callee]["scratch_insts"] == 0 and info[callee].get("ScratchSize", 0) == 0, (n, callee)


def test_riccati_rows_keeps_out_of_scratch(wide):
    s, _, info = wide
    rows = [n for n in info if "riccati_rows" in n]
    assert len(rows) == 2                                        # NH = 7 and NH = 6
    stats = isa_stats.functions(s)
    for n in rows:
        assert info[n]["scratch_insts"] == 0 and info[n].get("ScratchSize", 0) == 0, n
        assert not [op for op in stats[n] if op.startswith("scratch_")], n


def test_the_wide_kernels_spill_no_vgpr(wide):
    _, rem, _ = wide
    kernels = {k: v for k, v in rem.items() if "tsat_solve_kernel" in k}
    assert len(kernels) == 12
    for k, v in kernels.items():
        assert int(v["VGPRs Spill"]) == 0, (k, v)
        assert int(v["VGPRs"]) == 256, (k, v)                    # the whole file, AGPRs on top: one wavefront per SIMD
