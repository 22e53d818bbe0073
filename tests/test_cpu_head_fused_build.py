"""-m "not gpu": the kernels with the head folded in, as they compile for gfx950.

csrc/trans_ws.hip instantiates trans_ws_kernel<NK, 64, 512, true> for NK = 16 (K = 1024, the network's last transition) and NK = 0
(run-time k-tile count), csrc/dense_block7.hip dense_block7_kernel<6, true>.  Both hold a CU alone - two waves per SIMD with 256
registers each, one wave per SIMD with 512 - and must not spill or touch scratch: read from the code-object metadata of a device-only
compile with the Makefile's flags.  Their LDS is dynamic (the metadata says 0 static bytes); the sizes the launchers ask for are
restated here from the sources' constants, which the sources hold under 160 KB with static_asserts of their own.  The instantiations
that existed before keep their names apart from the new template argument."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tennis_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_MAX = 160 * 1024


def _hflags():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    flags = re.search(r"^HFLAGS := \$\(EXTRA\) (.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    d = tmp_path_factory.mktemp("head_fused_isa")
    procs = {}
    for unit in ("trans_ws", "dense_block7"):
        out = str(d / (unit + ".s"))
        procs[unit] = (out, subprocess.Popen([HIPCC] + _hflags() + ["--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", out],
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    texts = {}
    for unit, (out, p) in procs.items():
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, log[-4000:]
        texts[unit] = open(out).read()
    return texts


def _meta(text):
    """{demangled-enough kernel name: {field: int}} from the amdhsa.kernels metadata"""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        f = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}
        f["agpr_count"] = int(re.match(r"\s*(\d+)", blk).group(1))
        out[name] = f
    return out


def _clean(f, vgpr_max):
    assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, f
    assert f["group_segment_fixed_size"] == 0, f             # dynamic LDS only
    assert f["vgpr_count"] <= vgpr_max and f["max_flat_workgroup_size"] in (256, 512), f


def test_transition_instantiations(listings):
    text = listings["trans_ws"]
    meta = _meta(text)
    kern = {n: f for n, f in meta.items() if "trans_ws_kernel" in n}
    # trans_ws_kernelILi<NK>ELi<BM>ELi<NB>ELb<HEAD>E
    got = sorted(tuple(int(v) for v in re.search(r"trans_ws_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E", n).groups()) for n in kern)
    assert got == [(0, 64, 512, 0), (0, 64, 512, 1), (0, 128, 256, 0), (8, 128, 256, 0), (16, 64, 512, 0), (16, 64, 512, 1)], got
    for n, f in kern.items():
        _clean(f, 256)                                       # two waves per SIMD
        assert f["max_flat_workgroup_size"] == 512
    assert "scratch_" not in text
    src = open(os.path.join(CSRC, "trans_ws.hip")).read()
    assert "constexpr int kHeadRows = 49;" in src and "constexpr int kHeadTermPitch = 512 * 4 + 16;" in src
    assert "constexpr int kHeadTermOff = kHeadRows * TG<64, 512>::CPITCH;" in src and "static constexpr int CPITCH = NB * 2 + 16;" in src
    assert "constexpr int kHeadLdsBytes = kHeadTermOff + kHeadRows * kHeadTermPitch;" in src
    lds = 49 * (512 * 2 + 16) + 49 * (512 * 4 + 16)
    assert lds == 152096 <= LDS_MAX
    assert "kHeadLdsBytes <= 160 * 1024" in src


def test_block7_instantiations(listings):
    text = listings["dense_block7"]
    meta = _meta(text)
    kern = {n: f for n, f in meta.items() if "dense_block7_kernel" in n}
    got = sorted(tuple(int(v) for v in re.search(r"dense_block7_kernelILi(\d+)ELb(\d)E", n).groups()) for n in kern)
    assert got == [(6, 0), (6, 1)], got
    for n, f in kern.items():
        _clean(f, 512)                                       # one wave per SIMD with the whole register file
        assert f["max_flat_workgroup_size"] == 256
    assert "scratch_" not in text
    src = open(os.path.join(CSRC, "dense_block7.hip")).read()
    base = 128 * 49 * 16 + 51 * 272 + 4 * 8192 + (512 + 512 + 128) * 4          # kLdsBytes: activations, bottleneck tile, reduction, tables
    assert "constexpr int kHeadOff = kLdsBytes, kHeadPitch = 52 * 4;" in src and "constexpr int kLdsBytesHead = kHeadOff + 32 * kHeadPitch;" in src
    assert base == 151600 and base + 32 * 52 * 4 == 158256 <= LDS_MAX
    assert "kLdsBytesHead <= 160 * 1024" in src
