"""The replay model shared by tests/test_cpu_block14.py and tests/test_cpu_block28.py: one wave's vector-memory issue order in the
streamed block kernels.

vmcnt(N) returns when at most N loads are outstanding, and loads complete in order, so a wait is correct iff at least N loads
were issued BEHIND the one it needs.  `Wave` counts the loads and checks every wait.  `Wave.su_interval` replays the 32 slots of a
1x1 super-step interval: it mirrors dense_block14.hip::su_interval AND dense_block28.hip::su_interval, which issue their loads in
the same order but are still two copies - a change of the slot layout in either has to be made in both and mirrored here.  The
statements themselves (ring_wait, ring_load, the DMA statements) and the shared constants are in tennis_amd/csrc/dense_stream.h.
The stage structure (layers with a tail interval / (layer, pass) stages) is the kernels' own and stays in the two test files."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tennis_amd", "csrc")


def constants(kernel_file, needed):
    """The kVm*, kNR and kPreItems constants out of the text the compiler reads: dense_stream.h plus the kernel's own file.
    Nothing is restated here: a name in `needed` that neither file defines is an error."""
    text = open(os.path.join(CSRC, "dense_stream.h")).read() + open(os.path.join(CSRC, kernel_file)).read()
    c = {k: int(v) for k, v in re.findall(r"\b(kVm\w+) = (\d+)", text)}
    for k in ("kNR", "kPreItems"):
        m = re.search(r"constexpr int %s = (\d+)" % k, text)
        if m:
            c[k] = int(m.group(1))
    missing = [k for k in needed if k not in c]
    assert not missing, f"{missing} defined neither in dense_stream.h nor in {kernel_file}"
    return c


class Wave:
    def __init__(self, c):
        self.c = c
        self.n = 0                      # loads issued so far
        self.done_upto = 0              # loads [0, done_upto) known complete (a vmcnt(0))
        self.ring = {}                  # (rs, kq, f) -> (issue index, what it holds: (layer or stage, su, kq))
        self.dma = {}                   # unit -> issue index of this wave's LAST piece
        self.next_unit = 0              # unit the next DMA statements copy
        self.min_slack = {}

    def load(self):
        self.n += 1
        return self.n - 1

    def need(self, idx, vm, what):
        younger = self.n - 1 - idx
        ok = idx < self.done_upto or younger >= vm
        assert ok, f"{what}: vmcnt({vm}) with only {younger} loads behind the one it waits for"
        if idx >= self.done_upto:
            k = what.split(":")[0]
            self.min_slack[k] = min(self.min_slack.get(k, 1 << 30), younger - vm)

    # -- the kernels' statements
    def dma_pair(self):
        self.load(); self.load()

    def dma_consts(self):
        self.dma[self.next_unit] = self.load()
        self.next_unit += 1             # (advance_dma at the end of the interval; nothing copies in between)

    def ring_load(self, rs, kq, f, holds):
        self.ring[(rs, kq, f)] = (self.load(), holds)

    def ring_wait(self, rs, kq, expect):
        for f in (0, 1):
            idx, holds = self.ring[(rs, kq, f)]
            assert holds == expect, f"ring[{rs}][{kq}][{f}] holds {holds}, its consumer expects {expect}"
            self.need(idx, self.c["kVmRing"], "ring: %s" % (expect,))

    def begin_interval(self, g, vm):
        assert g + 1 in self.dma, f"unit {g + 1} was never copied"
        self.need(self.dma[g + 1], vm, "dma: unit %d" % (g + 1))      # this wave's pieces of unit g + 1

    def su_interval(self, g, rs, kind, here, nxt, ta, tb):
        """su_interval: unit g = super-step `here` = (stage, u) in ring slot rs; kind 0 first / 1 inner / 2 last of its stage.
        `nxt` = the super-step behind it, (stage, u) (kind 2 produces none of its k-steps); ta / tb = (stage, u) of the refill
        targets rb_a (k-steps 1 .. 3) / rb_b (k-step 0)."""
        c = self.c
        self.begin_interval(g, c["kVmDmaSU0"] if kind == 0 else c["kVmDmaSU"])
        for q in range(4):
            for e in range(8):
                j, bf = e >> 1, e & 1
                if q < 3:
                    if e == 0:
                        self.ring_wait(rs, q + 1, here + (q + 1,))
                    if j == 3:
                        self.ring_load(rs, q + 1, bf, ta + (q + 1,))
                elif kind != 2:
                    if e == 0:
                        self.ring_wait(rs ^ 1, 0, nxt + (0,))
                    if j == 3:
                        self.ring_load(rs ^ 1, 0, bf, tb + (0,))
                if e == 7:
                    if q in (0, 1):
                        self.dma_pair()
                    elif q == 3:
                        self.dma_consts()
