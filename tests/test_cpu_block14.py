"""-m "not gpu": the hand-counted s_waitcnt vmcnt(N) constants of dense_block14.hip (and of the core it shares with
dense_block28.hip, dense_stream.h), proven by replaying the kernel's issue order.

The 14x14 block kernel issues every steady-state vector-memory load from inline asm (the activation ring's refills and the
LDS-DMA pieces of the weight stream) and waits for them with literal counts: vmcnt(N) returns when at most N loads are
outstanding, and loads complete in order, so a wait is correct iff at least N loads were issued BEHIND the one it needs.  This
test re-states the issue order of one wave for whole blocks (every interval kind, both ring parities, odd and even super-step
counts), takes the constants from the source, and checks every wait - plus that each ring register holds the super-step and
k-step its consumer expects.  It is a model of the schedule, kept next to it: a change of the slot layout in the kernel has to
be mirrored here and in tests/tools/vmcnt_replay.py, which holds the wave model and the replay of a super-step interval (the
comments name the kernel's statements)."""
import pytest

from tools.vmcnt_replay import Wave, constants as _constants


def constants():      # (the shared ones from dense_stream.h, kVmDmaTail / kVmDmaB0 from the kernel's own file)
    return _constants("dense_block14.hip", ["kVmRing", "kVmDmaSU0", "kVmDmaSU", "kVmDmaTail", "kVmDmaB0", "kVmDmaB", "kNR", "kPreItems"])


def nsu_of(K):
    return (K - 32 + 63) // 64


def run_block(K0, nl, c):
    w = Wave(c)
    # prologue: units 0 .. 3, the first layer's super-steps 0 / 1, vmcnt(0), the head of the pipeline (pre_item)
    for _ in range(4):
        w.dma_pair(); w.dma_pair(); w.dma_consts()
    for rs in (0, 1):
        for kq in range(4):
            for f in (0, 1):
                w.ring_load(rs, kq, f, (0, rs, kq))
    w.done_upto = w.n

    def wrap(l, su):                     # super-step su of layer l, or of the layers behind it
        while su >= nsu_of(K0 + 32 * l):
            su -= nsu_of(K0 + 32 * l)
            l += 1
        return l, su

    def pre_items(pn, l):                # b_interval J = 5 / prologue: BN of (layer l, super-step 0, k-step 0); refill <- super-step 2, k-step 0
        w.ring_wait(pn, 0, (l, 0, 0))
        for f in (0, 1):
            w.ring_load(pn, 0, f, (l, 2, 0))
    pre_items(0, 0)
    w.done_upto = w.n                    # (the prologue waits for its two refills: no DMA statements follow them there)
    g, par = 0, 0
    for l in range(nl):
        nsu = nsu_of(K0 + 32 * l)
        assert nsu >= 4
        for u in range(nsu):             # su_interval
            kind = 0 if u == 0 else (2 if u == nsu - 1 else 1)
            w.su_interval(g, (u + par) & 1, kind, (l, u), (l, u + 1), wrap(l, u + 2), wrap(l, u + 3))
            g += 1
        # tail_interval
        w.begin_interval(g, c["kVmDmaTail"])
        w.dma_pair(); w.dma_pair(); w.dma_consts()
        g += 1
        par = (par + nsu) & 1
        for j in range(6):               # b_interval
            w.begin_interval(g, c["kVmDmaB0"] if j == 0 else c["kVmDmaB"])
            if j == 5:
                assert c["kPreItems"] <= 15      # the head of the next layer's pipeline sits in front of the interval's DMA statements
                pre_items(par, l + 1)
            w.dma_pair(); w.dma_pair(); w.dma_consts()
            g += 1
    return w, g


@pytest.mark.parametrize("K0,nl", [(256, 24), (512, 16), (256, 1), (288, 5), (320, 8)])
def test_vmcnt_constants_hold_for_every_wait(K0, nl):
    c = constants()
    w, units = run_block(K0, nl, c)
    assert units == sum(nsu_of(K0 + 32 * l) + 7 for l in range(nl))
    assert w.next_unit == units + 4              # the stream carries four units of padding for the last intervals' copies
    # the counts are not only safe but tight enough to keep the prefetch distance: a ring load may stay in flight for (almost) its two intervals
    assert w.min_slack["ring"] <= 2, w.min_slack
    assert w.min_slack["dma"] <= 8, w.min_slack


def test_a_wrong_constant_is_caught():
    c = constants()
    c["kVmRing"] += 8
    with pytest.raises(AssertionError, match="vmcnt"):
        run_block(256, 24, c)
    c = constants()
    c["kVmDmaB"] += 6
    with pytest.raises(AssertionError, match="vmcnt"):
        run_block(256, 24, c)
