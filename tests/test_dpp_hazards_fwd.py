"""CPU tier: the DPP data hazards of the forward sweep's feedback block (TSAT_FG_6 / TSAT_FG_7, tsat_riccati_dpp.inc), checked
statically in the ISA hipcc generates (tools/check_dpp_hazards.py) for the wide unit — the only one that compiles the block: it
inlines the sweep into the kernel, two register sets taking turns, and the packed unit that tests/test_dpp_hazards.py compiles
does not contain it. The block's DPP operands are the two doubles of the knot's gain record a lane has read from LDS; whatever
the compiler moves them through on the way — a copy, an AGPR read — must lie two wait states back, which the block's opening
s_nop sees to."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_dpp_hazards as chk  # noqa: E402


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_forward_feedback_block_has_no_dpp_hazard(tmp_path):
    unit = "tsat_kernels.hip"
    assert unit in chk.ALL_UNITS            # (what `check_dpp_hazards.py --all` walks as well)
    out = str(tmp_path / (unit + ".s"))
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", os.path.join(chk.CSRC, unit), "-o", out],
                          stderr=subprocess.DEVNULL)
    # the block is there: lanes 10 and 11 of a row are named by the forward sweep's d terms alone (the Riccati rows stop at lane 9)
    with open(out) as f:
        n_fwd = len(re.findall(r"v_fmac_f64_dpp .* row_newbcast:11 ", f.read()))
    assert n_fwd > 0 and n_fwd % 2 == 0
    n, bad = chk.check_listing(out)
    assert n > 0 and bad == [], bad[:10]
