"""What a step workspace holds between simulate() calls, and what a call with given FnxStepParams.static_flags trusts of it: a plain
restatement of step_plan and stage_word_plan (fluidnet_cxx_amd/csrc/fnx_step_plan.h) for a state that has a BC array and a workspace
of FNX_OP_STEP_STATIC's size (the automatic mode's: in 3D the stage word map exists).

Contents are named by GENERATIONS, numbers the caller hands out: a new one whenever the contents of flags, or of any BC array, change
-- an in-place write, another tensor, a new tensor at an old address.  Nothing here looks at addresses or version counters, so a
recycled address is a different generation.  None stands for unknown or garbage: a fresh workspace, or what a call that raised was
about to build (it may have written half of it).

    ws = Workspace(is3d)
    bad = ws.check(bits, method, g_flags, g_bc)      # what these bits trust but the workspace does not hold; [] when sound
    ws.call(bits, method, g_flags, g_bc, ok)         # the call has run (ok) or raised (not ok)

Bits: 1 = flags unchanged, 2 = BC arrays unchanged (go by the class map), 4 = the class map is built, 8 = the PCG hierarchy is kept."""

METHODS = ("jacobi", "convnet", "pcg", "hybrid")
# Mixed methods on one set of tensors with one in-place write to flags (wf) and one to a BC array (wb), no failing call and no recycled
# address, and the bits of its calls, 2D and 3D alike: those of the commit before the bookkeeping was made to record on success only.
PINNED = "J J J P P J C H J wf J P J wb C P J J"
PINNED_BITS = [0, 3, 7, 7, 15, 7, 7, 15, 7, 6, 7, 7, 1, 11, 7, 7]
NONE, BUILD, REUSE = "none", "build", "reuse"


def plan(bits, method, is3d):
    """{item: NONE | BUILD | REUSE} for the four kept things: what the call does not touch, derives again, or trusts"""
    assert method in METHODS, method
    p = dict(mask=NONE, cls=NONE, word=NONE, mg=NONE)
    if is3d and method == "jacobi":
        p["mask"] = REUSE if bits & 1 else BUILD                    # StepPlan.reuse_mask
    if bits & 2:
        p["cls"] = REUSE if bits & 4 else BUILD                     # StepPlan.class_map
    if is3d and p["cls"] != NONE:
        p["word"] = REUSE if (bits & 5) == 5 else BUILD             # stage_word_plan
    if method in ("pcg", "hybrid"):
        p["mg"] = REUSE if (bits & 9) == 9 else BUILD               # StepPlan.pcg_rebuild
    return p


class Workspace:
    def __init__(self, is3d):
        self.is3d = bool(is3d)
        self.mask = self.cls = self.word = self.mg = None           # the generations each kept thing was built from

    def _current(self, g_flags, g_bc):
        return dict(mask=g_flags, cls=g_bc, word=(g_flags, g_bc), mg=g_flags)

    def check(self, bits, method, g_flags, g_bc):
        """the items a call with these bits on flags / BC arrays of these generations trusts although the workspace does not hold them"""
        want = self._current(g_flags, g_bc)
        return [f"{item}: trusted for {want[item]}, the workspace holds {getattr(self, item)}"
                for item, what in plan(bits, method, self.is3d).items() if what == REUSE and getattr(self, item) != want[item]]

    def call(self, bits, method, g_flags, g_bc, ok=True):
        """a call that returns leaves behind what it built; one that raises leaves that unknown"""
        now = self._current(g_flags, g_bc)
        for item, what in plan(bits, method, self.is3d).items():
            if what == BUILD:
                setattr(self, item, now[item] if ok else None)
