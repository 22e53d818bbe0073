"""-m "not gpu": the build-time ISA audit (scripts/audit_strip_isa.py, `make audit`) on the CHAINED strip kernels.

dense_strip_kernel_chain<W> runs five (56 x 56) / six (28 x 28) layer bodies of dense_strip_body.h one behind the other in one kernel.  Every body keeps
the literal accumulator window a160-a255, and the widest bodies fill the register file on their own: what one layer leaves
live into the next turns into scratch spills (the K = 320 layer of the 28 x 28 block does spill as a seventh link, which is
why it is not one).  The audit finds the chained kernels by name; this test makes sure that it does, that they are clean,
that each holds all its layers, and that every layer boundary is there."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "tennis_amd", "csrc", "isa")
UNITS = ["dense_strip_chain_w56", "dense_strip_chain_w28"]
AUDIT = os.path.join(ROOT, "scripts", "audit_strip_isa.py")
NL = {"dense_strip_chain_w56": 5, "dense_strip_chain_w28": 6}          # layers per chained kernel (dense_strip_impl.h::DSChain)


def _listings():
    files = [os.path.join(ISA, u + ".s") for u in UNITS]
    if not all(os.path.exists(f) for f in files):
        subprocess.run(["make", "-C", ROOT, "-j8", "audit"], check=True, capture_output=True)
    return files


def test_audit_finds_the_chained_kernels_and_passes():
    r = subprocess.run([sys.executable, AUDIT] + _listings(), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"audited 2 kernels, 0 problem", r.stdout), r.stdout


def test_chained_kernels_have_no_scratch_and_all_their_layers():
    for f in _listings():
        nl = NL[os.path.basename(f)[:-2]]
        text = open(f).read()
        names = re.findall(r"^(\S*dense_strip_kernel_chain\S*):", text, re.M)
        assert len(names) == 1, (f, names)
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"], f
        assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"], f
        assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"], f
        assert "scratch_" not in text, f
        # a layer = one weight prologue (a loop of LDS-DMA pieces per operand) + one barrier behind it; a boundary = one more
        # barrier, directly behind the wait for the wave's own stores and LDS reads
        assert len(re.findall(r"s_waitcnt vmcnt\(0\) lgkmcnt\(0\)\n\ts_barrier", text)) == nl - 1, f
        assert len(re.findall(r"^\ts_barrier", text, re.M)) == 2 * nl - 1, f
