"""-m "not gpu": the build-time ISA audit (scripts/audit_strip_isa.py, `make audit`) on the PAIRED strip kernels of the 28 x 28 maps.

csrc/dense_strip_pair_w28.hip instantiates the layer body of dense_strip_body.h with the geometry DSGeomPair<KS> - two frames per
workgroup, 14 rows per wave - as dense_strip_pair_kernel<KS>, KS = 4 ... 10, and six of them (K = 128 ... 288) one behind the other
as dense_strip_pair_kernel_chain.  Every body keeps the literal accumulator window a160-a255, and the widest fill the register
file; the 14-row loop with its extra row event costs registers the 7-row form does not (the K = 288 and K = 320 bodies went to
scratch until their weight-fragment reads got base registers of their own).  The audit finds the kernels by name; this test makes
sure that it does, that they are clean, that nothing spills, and that the chained kernel holds all its layers and boundaries."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "tennis_amd", "csrc", "isa")
UNIT = "dense_strip_pair_w28"
AUDIT = os.path.join(ROOT, "scripts", "audit_strip_isa.py")
NL = 6                      # layers of the chained kernel (dense_strip_impl.h::DSChain<28>)
KS = range(4, 11)           # the per-layer instantiations


def _listing():
    f = os.path.join(ISA, UNIT + ".s")
    if not os.path.exists(f):
        subprocess.run(["make", "-C", ROOT, "-j8", "audit"], check=True, capture_output=True)
    return f


def _kernels(text):
    """{mangled name: its text from the label to .end_amdhsa_kernel}"""
    out = {}
    for m in re.finditer(r"^(\S*dense_strip_pair_kernel\S*):", text, re.M):
        out[m.group(1)] = text[m.end():text.find(".end_amdhsa_kernel", m.end())]
    return out


def test_audit_finds_the_paired_kernels_and_passes():
    r = subprocess.run([sys.executable, AUDIT, _listing()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"audited 8 kernels, 0 problem", r.stdout), r.stdout


def test_every_instantiation_is_there_once():
    names = sorted(_kernels(open(_listing()).read()))
    assert len([n for n in names if "dense_strip_pair_kernel_chain" in n]) == 1, names
    for ks in KS:
        assert len([n for n in names if "dense_strip_pair_kernelILi%dEE" % ks in n]) == 1, (ks, names)
    assert len(names) == 8, names


def test_no_scratch_and_no_spills():
    text = open(_listing()).read()
    assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text) == ["0"] * 8
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", text) == ["0"] * 8
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * 8
    assert re.findall(r";\s*ScratchSize:\s*(\d+)", text) == ["0"] * 8
    assert "scratch_" not in text
    # one wave per SIMD with the whole register file: never more than 512 registers, and the window is above everything hipcc allocates
    counts = [int(c) for c in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    assert len(counts) == 8 and max(counts) <= 512, counts


def test_chained_kernel_has_all_its_layers_and_boundaries():
    kern = _kernels(open(_listing()).read())
    (chain,) = [t for n, t in kern.items() if "dense_strip_pair_kernel_chain" in n]
    # a layer = one weight prologue + one barrier behind it; a boundary = one more barrier, directly behind the wait for the
    # wave's own stores and LDS reads: 5 boundary barriers, 11 in all
    assert len(re.findall(r"s_waitcnt vmcnt\(0\) lgkmcnt\(0\)\n\ts_barrier", chain)) == NL - 1
    assert len(re.findall(r"^\ts_barrier", chain, re.M)) == 2 * NL - 1
    # and a per-layer kernel has the one barrier behind its prologue
    for n, t in kern.items():
        if "chain" not in n:
            assert len(re.findall(r"^\ts_barrier", t, re.M)) == 1, n
