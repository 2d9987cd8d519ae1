"""The automatic mode of the four-argument simulate() call without a GPU: the real `_AutoStep` of fluidnet_cxx_amd/_simulate.py is driven
through sequences of events on CPU tensors (their (data_ptr, _version, shape, stride) are what it goes by), and after every call the
bits it gave are checked against static_inputs_model: no bit may trust what the workspace does not hold.

A step is `bits, after = entry.begin(...)`, the native call, `entry.commit(after)` -- here the native call is nothing (X+) or an
exception, i.e. no commit (X-).  Events, one token each:
  J+ P+ C+ H+   a 'jacobi' / 'pcg' / 'convnet' / 'hybrid' call that returns          J- P- C-   one that raises
  wf  wb        an in-place write to flags / to one BC array
  nf            a new flags tensor with new contents (the old one is dropped)
  sf  sb        swap between two live flags tensors / two live sets of BC arrays
  rf  rb        the caller drops the flags tensor / one BC array in use and makes a new one with new contents, which lies where the
                allocator would put it: at the old one's address with a fresh version counter if the old one is freed by then (the
                entry does not hold it), else somewhere new
  fg            forget_static_inputs()
  fr            a fresh _AutoStep with a fresh workspace (what release_workspaces() or an eviction gives)"""
import itertools
import random
import weakref

import numpy as np
import pytest
import torch

from static_inputs_model import PINNED, PINNED_BITS, Workspace

CALLS = {"J": "jacobi", "P": "pcg", "C": "convnet", "H": "hybrid"}
CALL_EVENTS = ("J+", "P+", "C+", "H+", "J-", "P-", "C-")
EVENTS = CALL_EVENTS + ("wf", "wb", "nf", "sf", "sb", "rf", "rb", "fg", "fr")
BC_KEYS = ("UBC", "UBCInvMask", "densityBC", "densityBCInvMask")
SHAPE = (1, 1, 1, 2, 2)
MAXLEN = 4      # all 16 events to length 5 take about 40 s a dimension; length 4 and the random sequences of 12 take 5 s


class Slot:
    """one tensor over a numpy buffer of its own, and the generation of its contents"""

    def __init__(self, world, buf=None):
        self.buf = np.zeros(SHAPE, np.float32) if buf is None else buf
        self.buf += 1.0                              # (other contents, through numpy: no version counter sees it)
        self.t = torch.from_numpy(self.buf)          # (over an old buffer: the old address with a fresh version counter)
        self.g = world.generation()

    def recycled(self, world):
        """The caller drops this tensor and makes a new one with other contents.  Where nothing else held the old one (the entry under
        test, that is) it is freed and the allocator hands its block out again: the same address, a fresh version counter.  Where
        something does, the address is taken and the new tensor lies elsewhere."""
        alive = weakref.ref(self.t)
        self.t = None
        return Slot(world, self.buf if alive() is None else None)


class World:
    """the caller's tensors, the entry under test and the model of its workspace"""

    def __init__(self, sim, is3d):
        self.sim, self.is3d = sim, is3d
        self.count = 0
        self.flags = [Slot(self), None]              # two live flags tensors (the second from the first swap on), [0] is the one in use
        self.bcs = [[Slot(self) for _ in BC_KEYS], None]
        self.bc_g = [self.generation(), None]        # generation of each SET of BC arrays
        self.fresh_entry()
        self.bits = []

    def generation(self):
        self.count += 1
        return self.count

    def fresh_entry(self):
        self.entry = self.sim._AutoStep(16, torch.zeros(1))
        self.ws = Workspace(self.is3d)

    def do(self, ev):
        """one event; for a call, the list of what its bits wrongly trust"""
        if ev in CALL_EVENTS:
            method, ok = CALLS[ev[0]], ev[1] == "+"
            bd = {k: s.t for k, s in zip(BC_KEYS, self.bcs[0])}
            bits, after = self.entry.begin(bd, self.flags[0].t, self.is3d, method == "jacobi", method in ("pcg", "hybrid"))
            if ok:
                self.entry.commit(after)
            del after, bd
            self.bits.append(bits)
            gf, gb = self.flags[0].g, self.bc_g[0]
            bad = self.ws.check(bits, method, gf, gb)
            self.ws.call(bits, method, gf, gb, ok)
            return bad
        if ev == "wf":
            self.flags[0].t.add_(1.0)
            self.flags[0].g = self.generation()
        elif ev == "wb":
            self.bcs[0][0].t.mul_(1.5)
            self.bc_g[0] = self.generation()
        elif ev == "nf":
            self.flags[0] = Slot(self)
        elif ev == "sf":
            self.flags.reverse()
            if self.flags[0] is None:
                self.flags[0] = Slot(self)
        elif ev == "sb":
            self.bcs.reverse(); self.bc_g.reverse()
            if self.bcs[0] is None:
                self.bcs[0], self.bc_g[0] = [Slot(self) for _ in BC_KEYS], self.generation()
        elif ev == "rf":
            self.flags[0] = self.flags[0].recycled(self)
        elif ev == "rb":
            self.bcs[0][1] = self.bcs[0][1].recycled(self)
            self.bc_g[0] = self.generation()
        elif ev == "fg":
            self.sim._AUTO["host test"] = self.entry
            try:
                self.sim.forget_static_inputs()
            finally:
                del self.sim._AUTO["host test"]
        elif ev == "fr":
            self.fresh_entry()
        else:
            raise ValueError(ev)
        return []


def run(sim, is3d, seq):
    """(bits of the calls, None) or (bits so far, (index of the failing event, what it wrongly trusts))"""
    w = World(sim, is3d)
    for i, ev in enumerate(seq):
        bad = w.do(ev)
        if bad:
            return w.bits, (i, bad)
    return w.bits, None


def shrink(sim, is3d, seq):
    """a failing sequence with events taken out while it still fails"""
    seq = list(seq)
    again = True
    while again:
        again = False
        for i in range(len(seq)):
            shorter = seq[:i] + seq[i + 1:]
            _, fail = run(sim, is3d, shorter)
            if fail:
                seq, again = shorter[:fail[0] + 1], True
                break
    return seq


def report(sim, is3d, seq):
    seq = shrink(sim, is3d, seq)
    bits, (i, bad) = run(sim, is3d, seq)
    return f"{'3D' if is3d else '2D'} {' '.join(seq)}: bits {bits}, the last call trusts what the workspace does not hold -- " + "; ".join(bad)


@pytest.fixture(scope="module")
def sim():
    from fluidnet_cxx_amd import _simulate
    return _simulate


@pytest.mark.parametrize("is3d", [False, True], ids=["2d", "3d"])
def test_every_short_sequence_and_random_long_ones(sim, is3d):
    """Every sequence of up to MAXLEN events that ends in a call, shortest first, then 2 * 10^4 seeded random sequences of 12 events: no
    call trusts what the workspace does not hold.  The first failure is reported, shrunk to the shortest sequence found."""
    for n in range(1, MAXLEN + 1):
        for head in itertools.product(EVENTS, repeat=n - 1):
            for last in CALL_EVENTS:
                _, fail = run(sim, is3d, head + (last,))
                assert not fail, report(sim, is3d, head + (last,))
    rng = random.Random(20 + is3d)
    for _ in range(20000):
        seq = rng.choices(EVENTS, k=12)
        _, fail = run(sim, is3d, seq)
        assert not fail, report(sim, is3d, seq[:fail[0] + 1])


@pytest.mark.parametrize("is3d", [False, True], ids=["2d", "3d"])
def test_the_static_path_costs_nothing(sim, is3d):
    """In every run of up to six successful calls with nothing written between them the second call carries bits 0 and 1, the third bit
    2 as well, and the second and later PCG or hybrid calls bit 3.  One call cannot carry bit 0, and must not: a 3D Jacobi call before
    which no Jacobi call has built the mask."""
    for n in range(2, 7):
        for seq in itertools.product("JPCH", repeat=n):
            bits, fail = run(sim, is3d, [m + "+" for m in seq])
            assert not fail, report(sim, is3d, [m + "+" for m in seq])
            for i, (m, b) in enumerate(zip(seq, bits)):
                want = (0, 3, 7)[min(i, 2)]
                if is3d and m == "J" and "J" not in seq[:i]:
                    want &= ~1
                if m in "PH" and any(e in "PH" for e in seq[:i]):
                    want |= 8
                assert b == want, (seq, bits, i)


@pytest.mark.parametrize("is3d", [False, True], ids=["2d", "3d"])
def test_the_pinned_sequence_keeps_its_bits(sim, is3d):
    """mixed methods with one write to flags and one to a BC array, no failing call and no recycling: the bits of the commit before"""
    bits, fail = run(sim, is3d, [e + "+" if e in CALLS else e for e in PINNED.split()])
    assert not fail and bits == PINNED_BITS, (bits, fail)


# A call that raises left promises behind, and the identities of the mask's and the hierarchy's flags outlived their tensors: the
# shortest sequences on which the last call carried a wrong bit, with the bits they give now (None: 2D and 3D differ there, a 2D
# Jacobi call has no mask to wait for) and the last call's wrong bits before (`was`).  After a failed call the next one sends 0.
# A, B: the two live flags tensors ('sf' goes from one to the other); 'sf rf' goes back to A, drops it and makes A2 at its address.
NAMED = [
    ("3", "J- J+", [0, 0], 3),                                       # promised, never built: the mask
    ("23", "J+ J- J+", [0, 3, 0], 7),                                # the class map (3D: and the stage words)
    ("3", "P+ P- J+", [0, 11, 0], 6),                                # the class map
    ("3", "P+ P+ J- P+", [0, 11, 6, 0], 15),                         # the stage words
    # not recording the failed call is not enough: A, A, the BC set B fails half-way through rebuilding the class map, back to A --
    # the identities recorded last still say A (`was`: what such a fix gives)
    ("23", "J+ J+ sb J- sb J+", [0, 3, 1, 0], 7),
    ("3", "J+ sf P+ sf rf P+ J+", [0, 2, 6, 6], 7),                  # J(A) P(B) del A P(A2) J(A2): the mask built from A
    ("23", "P+ sf J+ sf rf J+ P+", [0, 2, 6, 7], 15),                # P(A) J(B) del A J(A2) P(A2): the hierarchy built from A
    # ... J(B) del A2 J(A3) P(A3) after the first of the two: the hierarchy built from A2
    ("23", "J+ sf P+ sf rf P+ J+ sf J+ sf rf J+ P+", [0, 2, 6, None, 6, 6, 7], 15),
]


@pytest.mark.parametrize("dims,seq,want,was", NAMED, ids=[s.replace(" ", "") for _, s, _, _ in NAMED])
def test_named_counterexamples(sim, dims, seq, want, was):
    for is3d in (False, True):
        if "23"[is3d] not in dims:
            continue
        bits, fail = run(sim, is3d, seq.split())
        assert not fail, report(sim, is3d, seq.split())
        assert len(bits) == len(want) and all(w is None or b == w for b, w in zip(bits, want)), (is3d, seq, bits)
        assert bits[-1] != was


def test_the_recycle_events_recycle(sim):
    """the world's own claim: 'rf' once the entry has let go of a tensor gives a tensor of the same identity with other contents, and
    while the entry holds the tensor, one at another address"""
    w = World(sim, True)
    for ev in ("J+", "sf", "P+", "sf"):
        w.do(ev)
    ident, g = sim._ident(w.flags[0].t), w.flags[0].g
    w.do("rf")
    assert sim._ident(w.flags[0].t) == ident and w.flags[0].g != g
    w.do("J+")
    w.do("rf")
    assert sim._ident(w.flags[0].t)[0] != ident[0]
