"""Training of the 2D pressure net, end to end on the device (reference pytorch/fluid_net_train.py:170-206 and run_epoch, :245-375).

    from fluidnet_cxx_amd.training import train, SceneSampler, fluidnet_loss

What the reference reads from a pre-computed Mantaflow data set is generated here while training: `SceneSampler` keeps B scenes --
random obstacles (fnx_scene_obstacles), a divergence-free turbulent velocity and a density (fnx_scene_turbulence) -- advancing in lock
step through the solver, and hands out (data, target) batches in the reference's layout: data (B,5,1,H,W) = [p of the previous step,
U before the projection, flags, density], target (B,4,1,H,W) = [p, U, density] of the converged ('pcg') projection.  `fluidnet_loss` is
the loss of fluid_net_train.py:276-285 with its gradient from one kernel (fnx_train_loss); `train` is run_epoch's body around
`FluidNetTrain` (or, with mconf['model'] = 'FluidNet', the 16-channel bank net's `FluidNetBankTrain`), torch.optim.Adam and
ReduceLROnPlateau with the reference's arguments.

torch carries the tensors (allocation, copies, concatenation, the optimiser); the arithmetic on fields is the extension's kernels.
Every random choice comes from the counter-based hash of the scene kernels (include/fluidnet_hip.h), evaluated on the host for the
per-call choices: torch's global generator is never used, and one seed gives the same batches and the same trained bits.

2D only, like FluidNetTrain: a 3D grid is refused before the device is touched.  fluidnet_cxx_amd/training3d.py is the 3D counterpart;
the bodies that do not depend on the dimension stand here once, in private bases (_SceneSamplerBase, _train, _evaluate, _loss_fn) that
both modules use -- the precedent is train._FluidNetTrainBase -- and a `_Dim` record says what does depend on it.
"""
import copy


import torch

from . import fluid
from ._ext import ext
from ._simulate import simulate
from .train import FluidNetBankTrain, FluidNetTrain

# the scene generator's parameters (FnxSceneParams): up to four discs / boxes whose centres lie within 0.3 min(H, W) of the grid centre
# and whose radius / half extent is 0.03 .. 0.12 min(H, W) -- they never reach the border ring, and at least 70 % of the cells stay fluid
SCENE_DEFAULTS = dict(n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=4, wavelength=32.0,
                      amplitude=8.0, density_scale=1.0)
# trainConfig.yaml's modelParam (the keys training reads) + what the sampler and the loop need on top of it
MCONF_DEFAULTS = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
                      normalizeInputThreshold=1e-5, is3D=False, inputDim=2, lr=5e-5, pL2Lambda=0.0, divL2Lambda=1.0, pL1Lambda=0.0,
                      divL1Lambda=0.0, divLongTermLambda=1.0, longTermDivNumSteps=[4, 16], longTermDivProbability=0.9, dt=0.1,
                      buoyancyScale=0.0, gravityScale=0.0, gravityVec=dict(x=0.0, y=0.0, z=0.0), trainBuoyancyScale=2.0,
                      trainBuoyancyProb=0.3, correctScalar=False, operatingDensity=0.0, viscosity=0, timeScaleSigma=1.0,
                      maccormackStrength=0.6, sampleOutsideFluid=False, pcgTol=1e-5, pcgIter=50, pTol=0.0, jacobiIter=28)
TCONF_DEFAULTS = dict(res=128, batch=64, iters=1000, seed=0, sceneLength=32, stride=2, evalEvery=50, evalBatches=2, saveEvery=0)

_STREAM_SAMPLER, _STREAM_TRAINER = 64, 65      # host-side streams of the hash (the kernels use 0, 16 + octave and 32 + octave)


# ---- the hash on the host (include/fluidnet_hip.h; tests/scene_reference.py is the numpy statement, 2D and 3D) -----------------------
def _mix32(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def host_hash(seed, scene, stream, counter):
    return _mix32(_mix32(_mix32(_mix32(int(seed) + 0x9e3779b9) ^ (int(scene) & 0xffffffff)) ^ int(stream)) ^ (int(counter) & 0xffffffff))


def host_uniform(seed, scene, stream, counter):
    """(hash >> 8) * 2^-24 in [0, 1)"""
    return (host_hash(seed, scene, stream, counter) >> 8) * 2.0 ** -24


def host_normal(seed, scene, stream, counter):
    """a unit-variance, zero-mean variate: the sum of the 12 uniforms at counter .. counter + 11, minus 6 (additions only, so the value
    does not depend on a maths library)"""
    return sum(host_uniform(seed, scene, stream, counter + k) for k in range(12)) - 6.0


def lambdas_of(mconf):
    return [float(mconf.get(k, 0.0)) for k in ("pL2Lambda", "divL2Lambda", "pL1Lambda", "divL1Lambda")]


def _refuse_3d(what, *sizes):
    if any(int(s) != 1 for s in sizes):
        raise ValueError(f"fluidnet_cxx_amd.training.{what}: training is 2D only (depth {[int(s) for s in sizes]})")


# ---- what depends on the dimension ----------------------------------------------------------------------------------------------------
class _Dim:
    """what the loop needs to know about the dimension: `nU` velocity channels (data = [p, U (nU), flags, density]), the net's class, the
    sampler's constructor (mconf, B, dims, seed, device, scene, sceneLength, stride), the differentiable loss and the loss kernel's binding"""

    def __init__(self, nU, net, sampler, loss, raw_loss):
        self.nU, self.net, self.sampler, self.loss, self.raw_loss = nU, net, sampler, loss, raw_loss
        self.iU, self.iflags, self.irho = slice(1, 1 + nU), slice(1 + nU, 2 + nU), slice(2 + nU, 3 + nU)


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
def _loss_fn(raw_loss):
    """the autograd function around one loss kernel binding (ext.train_loss / ext.train_loss3d)"""

    class _LossFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, out_p, out_U, flags, target_p, lambdas):
            out_p, out_U = out_p.contiguous(), out_U.contiguous()
            terms5 = raw_loss(out_p, out_U, flags, target_p, lambdas, None, True)[0]
            ctx.save_for_backward(out_p, out_U, flags, target_p)
            ctx.lambdas = lambdas
            total, terms = terms5[4].clone(), terms5[:4].clone()
            ctx.mark_non_differentiable(terms)
            return total, terms

        @staticmethod
        def backward(ctx, g_total, _g_terms):
            out_p, out_U, flags, target_p = ctx.saved_tensors
            _, gp, gU = raw_loss(out_p, out_U, flags, target_p, ctx.lambdas, g_total.contiguous().reshape(1), False)
            return gp, gU, None, None, None

    return _LossFn


_LossFn = _loss_fn(ext.train_loss)


def fluidnet_loss(out_p, out_U, flags, target_p, lambdas):
    """fluid_net_train.py:276-285: (total, terms) with total = pL2Lambda mean (out_p - target_p)^2 + divL2Lambda mean div^2 + pL1Lambda
    mean |out_p - target_p| + divL1Lambda mean |div|, div = velocityDivergence(out_U, flags), and terms the four unweighted means (no
    gradient flows through them).  lambdas = (pL2, divL2, pL1, divL1); target_p may be None when both pressure lambdas are 0.
    Differentiable with respect to out_p and out_U: the backward is the same kernel with the upstream gradient as a device scalar."""
    lam = [float(v) for v in lambdas]
    assert len(lam) == 4, "lambdas = (pL2Lambda, divL2Lambda, pL1Lambda, divL1Lambda)"
    _refuse_3d("fluidnet_loss", flags.size(2))
    if target_p is not None:
        target_p = target_p.contiguous()
    return _LossFn.apply(out_p, out_U, flags.contiguous(), target_p, lam)


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
class _SceneSamplerBase:
    """B scenes advancing in lock step.  A subclass gives `_IS3D`, `draw(ids)` -> (flags, U, density) from its scene kernels and
    `_gravity(h)` -> (axis, sign) from one hash word."""

    _IS3D = False

    def _init(self, mconf, B, seed, device, scene_defaults, scene, sceneLength, stride):
        self.mconf = mconf
        self.B, self.seed = int(B), int(seed) & 0xffffffff
        self.device = torch.device(device)
        self.scene = dict(scene_defaults, **(scene or {}))
        self.sceneLength, self.stride = int(sceneLength), int(stride)
        assert self.B >= 1 and self.sceneLength >= 1 and self.stride >= 0
        self.age = [(b * self.sceneLength) // self.B for b in range(self.B)]
        self.scene_id = [-1] * self.B
        self.next_id = 0
        self.calls = 0
        self.last_choice = None
        self.last_redrawn = []
        self.bd = {}
        self._redraw(list(range(self.B)), keep_age=True)

    def _project(self, U, flags):
        div = fluid.velocityDivergence(U, flags)
        p, _ = fluid.solveLinearSystemPCG(flags, div, self._IS3D, self.mconf["pcgTol"], self.mconf["pcgIter"])
        fluid.velocityUpdate(p, U, flags)
        fluid.setWallBcs(U, flags)
        return p

    def _redraw(self, slots, keep_age=False):
        ids = list(range(self.next_id, self.next_id + len(slots)))
        self.next_id += len(slots)
        flags, U, rho = self.draw(ids)
        fluid.setWallBcs(U, flags)
        p = self._project(U, flags)
        new = dict(p=p, U=U, flags=flags, density=rho)
        if len(slots) == self.B:
            self.bd = new
        else:
            idx = torch.tensor(slots, dtype=torch.int64, device=self.device)
            for k, v in new.items():
                self.bd[k].index_copy_(0, idx, v)
        for b, i in zip(slots, ids):
            self.scene_id[b] = i
            if not keep_age:
                self.age[b] = 0
        self.last_redrawn = list(slots)

    def redraw_due(self):
        """redraws the slots whose scene has reached sceneLength; returns them"""
        due = [b for b in range(self.B) if self.age[b] >= self.sceneLength]
        if due:
            self._redraw(due)
        else:
            self.last_redrawn = []
        return due

    # -- per-call choices
    def choices(self, call):
        m, s = self.mconf, self.seed
        buoyancy = float(m["buoyancyScale"])
        if host_uniform(s, call, _STREAM_SAMPLER, 0) < m["trainBuoyancyProb"]:
            buoyancy = float(m["trainBuoyancyScale"]) + host_normal(s, call, _STREAM_SAMPLER, 16)
        axis, sign = self._gravity(host_hash(s, call, _STREAM_SAMPLER, 1))
        gvec = dict(x=0.0, y=0.0, z=0.0)
        gvec[axis] = sign
        dt = float(m["dt"])
        if m["timeScaleSigma"] > 0:
            dt = dt * (0.2028 + abs(host_normal(s, call, _STREAM_SAMPLER, 32)) * float(m["timeScaleSigma"]))
        return dict(dt=dt, buoyancyScale=max(buoyancy, 0.0), gravityVec=gvec)

    def sim_conf(self, choice):
        m = self.mconf
        conf = {k: m[k] for k in ("maccormackStrength", "sampleOutsideFluid", "gravityScale", "viscosity", "correctScalar", "operatingDensity",
                                  "pTol", "jacobiIter", "pcgTol", "pcgIter", "normalizeInputThreshold")}
        conf.update(choice)
        return conf

    # -- batches
    def next(self):
        self.redraw_due()
        choice = self.choices(self.calls)
        self.calls += 1
        self.last_choice = choice
        conf = self.sim_conf(choice)
        for _ in range(self.stride):
            simulate(conf, self.bd, None, "pcg")
        bd = self.bd
        p, U, flags, rho = bd["p"], bd["U"], bd["flags"], bd["density"]
        dt = conf["dt"]
        # lib/simulate.py:75-133 up to the projection, operator by operator (there are no BC arrays: setConstVals has nothing to do)
        rho = fluid.advectScalar(dt, rho, U, flags, method="maccormackFluidNet", boundary_width=1,
                                 sample_outside_fluid=conf["sampleOutsideFluid"], maccormack_strength=conf["maccormackStrength"])
        U = fluid.advectVelocity(dt=dt, orig=U, U=U, flags=flags, method="maccormackFluidNet", boundary_width=1,
                                 maccormack_strength=conf["maccormackStrength"])
        if conf["buoyancyScale"] > 0:
            g = [-conf["buoyancyScale"] * conf["gravityVec"][a] for a in ("x", "y", "z")]
            fluid.addBuoyancy(U, flags, rho, g, conf["operatingDensity"], dt)
        fluid.setWallBcs(U, flags)
        data = torch.cat((p, U, flags, rho), 1)
        p = self._project(U, flags)
        target = torch.cat((p, U, rho), 1)
        bd["p"], bd["U"], bd["density"] = p, U, rho
        self.age = [a + self.stride + 1 for a in self.age]
        return data, target

    # -- checkpointing
    def state_dict(self):
        return dict(seed=self.seed, age=list(self.age), scene_id=list(self.scene_id), next_id=self.next_id, calls=self.calls,
                    fields={k: v.detach().cpu().clone() for k, v in self.bd.items()})

    def load_state_dict(self, sd):
        assert sd["seed"] == self.seed and len(sd["age"]) == self.B, "the sampler state belongs to another seed or batch size"
        self.age, self.scene_id, self.next_id, self.calls = list(sd["age"]), list(sd["scene_id"]), sd["next_id"], sd["calls"]
        self.bd = {k: v.to(self.device).contiguous() for k, v in sd["fields"].items()}


class SceneSampler(_SceneSamplerBase):
    """B scenes of H x W cells advancing in lock step.  Scene b has an age (solver steps since it was drawn); once it reaches
    `sceneLength` the slot is redrawn under the next unused scene id.  Ages start staggered (slot b at b sceneLength // B), so a batch
    mixes young and old scenes.

    A redraw: obstacles, turbulence and density from the scene kernels, setWallBcs, one 'pcg' projection.
    next(): `stride` full 'pcg' steps; then the stages of one more step up to the projection on the operator path (advection, buoyancy,
    setWallBcs) -> data; the 'pcg' projection -> target.  Per call, from the hash on the host: the gravity direction (+-x / +-y), with
    probability trainBuoyancyProb a buoyancy scale trainBuoyancyScale + n, and the time step dt (0.2028 + |n| timeScaleSigma), n the
    host_normal variate (fluid_net_train.py:296-339).  `last_choice` holds them for the caller (the trainer's rollout uses the same)."""

    def __init__(self, mconf, B, H, W, seed, device="cuda", scene=None, sceneLength=32, stride=2, depth=1):
        _refuse_3d("SceneSampler", depth)
        if mconf.get("is3D", False):
            raise ValueError("fluidnet_cxx_amd.training.SceneSampler: training is 2D only (is3D=True)")
        self.H, self.W = int(H), int(W)
        self._init(dict(MCONF_DEFAULTS, **mconf), B, seed, device, SCENE_DEFAULTS, scene, sceneLength, stride)

    # -- scenes
    def draw(self, ids):
        """(flags, U, density) of the scenes `ids`, as the kernels give them (no boundary condition applied)"""
        s = self.scene
        t = torch.tensor([int(i) for i in ids], dtype=torch.int32, device=self.device)
        flags = ext.scene_obstacles(t, self.H, self.W, self.seed, s["n_min"], s["n_max"], s["centre_min"], s["centre_max"], s["size_min"],
                                    s["size_max"])
        U, rho = ext.scene_turbulence(t, self.H, self.W, self.seed, s["octaves"], s["wavelength"], s["amplitude"], s["density_scale"], True)
        return flags, U, rho

    def _gravity(self, h):
        return ("x", "y")[h & 1], float(((h >> 1) & 1) * 2 - 1)


_DIM = _Dim(2, FluidNetTrain, lambda mconf, B, dims, *rest: SceneSampler(mconf, B, dims[0], dims[1], *rest), fluidnet_loss,
            ext.train_loss)
# the same with the reference's 16-channel bank net in the middle (mconf['model'] = 'FluidNet')
_DIM_BANK = _Dim(2, FluidNetBankTrain, _DIM.sampler, fluidnet_loss, ext.train_loss)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def kaiming_init(net, seed):
    """fluid_net_train.py:170-187: kaiming_uniform_ on every convolution weight (the biases are left as constructed), from a generator of
    its own seeded with `seed`"""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(".weight"):
                w = torch.empty(p.shape, dtype=torch.float32)
                torch.nn.init.kaiming_uniform_(w, generator=gen)
                p.copy_(w)
    return net


def _evaluate(dim, net, batches, lambdas):
    tot = []
    with torch.no_grad():
        for data, target in batches:
            flags = data[:, dim.iflags].contiguous()
            tp = target[:, 0:1].contiguous() if (lambdas[0] or lambdas[2]) else None
            p, U = net(data)
            t_out = dim.raw_loss(p, U, flags, tp, lambdas, None, True)[0]
            t_in = dim.raw_loss(p, data[:, dim.iU].contiguous(), flags, None, [0.0, 1.0, 0.0, 0.0], None, True)[0]
            tot.append((t_out, t_in))
    host = [(a.cpu().tolist(), b.cpu().tolist()) for a, b in tot]
    n = float(len(host))
    return dict(loss=sum(a[4] for a, _ in host) / n, divL2_out=sum(a[1] for a, _ in host) / n, divL2_in=sum(b[1] for _, b in host) / n)


def _train(dim, mconf, tconf, dims, device, out, resume, log):
    """the body of train() / train3d(): `dims` = (H, W) resp. (D, H, W), the configurations complete"""
    dev = torch.device(device)
    B, seed, iters = int(tconf["batch"]), int(tconf["seed"]), int(tconf["iters"])
    lam = lambdas_of(mconf)
    lt_lambda = float(mconf["divLongTermLambda"])
    say = log if log is not None else (lambda *_: None)

    net = dim.net(mconf)
    kaiming_init(net, seed)
    net.to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=float(mconf["lr"]))
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.6, patience=10, threshold=3e-4, threshold_mode="rel")
    sampler = dim.sampler(mconf, B, dims, seed, dev, tconf.get("scene"), tconf["sceneLength"], tconf["stride"])
    held = dim.sampler(mconf, B, dims, seed ^ 0x5eed5eed, dev, tconf.get("scene"), tconf["sceneLength"], tconf["stride"])
    held_out = [held.next() for _ in range(int(tconf["evalBatches"]))]
    it0, history = 0, []
    if resume is not None:
        ck = torch.load(resume, map_location="cpu", weights_only=False) if isinstance(resume, str) else resume
        net.load_state_dict(ck["state_dict"])
        opt.load_state_dict(ck["optimizer"])
        sched.load_state_dict(ck["scheduler"])
        sampler.load_state_dict(ck["sampler"])
        it0, history = int(ck["it"]), list(ck.get("history", []))

    def checkpoint(it):
        ck = dict(state_dict={k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, optimizer=copy.deepcopy(opt.state_dict()),
                  mconf=mconf, it=it, scheduler=copy.deepcopy(sched.state_dict()), sampler=sampler.state_dict(), tconf=tconf,
                  history=list(history))
        if out:
            torch.save(ck, out)
        return ck

    one = torch.ones((), device=dev)
    lt_weight = torch.full((), lt_lambda, device=dev)
    pending = []                                          # (it, total, long-term total or None, lr): read back in one go
    for it in range(it0, iters):
        data, target = sampler.next()
        opt.zero_grad()
        flags = data[:, dim.iflags].contiguous()
        target_p = target[:, 0:1].contiguous() if (lam[0] or lam[2]) else None
        out_p, out_U = net(data)
        total, _ = dim.loss(out_p, out_U, flags, target_p, lam)
        roots, weights, total_lt = [total], [one], None
        if lt_lambda > 0:
            # fluid_net_train.py:341-375: some steps into the future with the net as it is (no gradient), then the divergence the net
            # leaves there.  The sampler's choices of this call (time step, buoyancy, gravity direction) hold for the rollout too.
            steps = mconf["longTermDivNumSteps"]
            n = int(steps[1] if host_uniform(seed, it, _STREAM_TRAINER, 0) > mconf["longTermDivProbability"] else steps[0])
            bd = dict(p=out_p.detach().clone(), U=out_U.detach().clone(), flags=flags, density=data[:, dim.irho].contiguous())
            conf = sampler.sim_conf(sampler.last_choice)
            with torch.no_grad():
                for _ in range(n):
                    simulate(conf, bd, net, "convnet")
            data_lt = torch.cat((bd["p"], bd["U"], flags, bd["density"]), 1)
            p_lt, U_lt = net(data_lt)
            total_lt, _ = dim.loss(p_lt, U_lt, flags, None, [0.0, 1.0, 0.0, 0.0])
            roots.append(total_lt)
            weights.append(lt_weight)
        torch.autograd.backward(roots, weights)
        opt.step()
        pending.append((it, total.detach(), None if total_lt is None else total_lt.detach(), opt.param_groups[0]["lr"]))
        done = it + 1
        evaluating = tconf["evalEvery"] and done % int(tconf["evalEvery"]) == 0
        saving = tconf["saveEvery"] and done % int(tconf["saveEvery"]) == 0 and done != iters
        if evaluating or saving or done == iters:
            for i, a, b, lr in pending:
                history.append(dict(it=i, loss=float(a), lt=None if b is None else float(b), lr=lr))
            pending = []
        if evaluating:
            ev = _evaluate(dim, net, held_out, lam)
            sched.step(ev["loss"])
            history[-1].update(val=ev["loss"], val_divL2_out=ev["divL2_out"], val_divL2_in=ev["divL2_in"])
            say(f"it {done:6d}  loss {history[-1]['loss']:.4e}  long-term {history[-1]['lt']}  held-out {ev['loss']:.4e}  "
                f"divL2 out/in {ev['divL2_out'] / max(ev['divL2_in'], 1e-300):.4e}  lr {opt.param_groups[0]['lr']:.3e}")
        if saving:
            checkpoint(done)
    ck = checkpoint(iters)
    return dict(net=net, checkpoint=ck, history=history, held_out=held_out, sampler=sampler)


def evaluate(net, batches, lambdas):
    """held-out figures under no_grad, averaged over `batches` [(data, target)]: the loss, divL2 of the net's U and divL2 of the U it was
    given (before the projection)"""
    return _evaluate(_DIM, net, batches, lambdas)


def jacobi_divL2(batches, sweeps):
    """divL2 of the held-out U after a Jacobi projection of `sweeps` sweeps (the operator path of simulate()), averaged over the batches"""
    vals = []
    for data, _ in batches:
        flags, U = data[:, 3:4].contiguous(), data[:, 1:3].contiguous()
        div = fluid.velocityDivergence(U, flags)
        p, _ = fluid.solveLinearSystemJacobi(flags=flags, div=div, is_3d=False, p_tol=0.0, max_iter=int(sweeps))
        fluid.velocityUpdate(p, U, flags)
        fluid.setWallBcs(U, flags)
        vals.append(ext.train_loss(p, U, flags, None, [0.0, 1.0, 0.0, 0.0], None, True)[0])
    return sum(v.cpu().tolist()[1] for v in vals) / float(len(vals))


def jacobi_sweeps_to_reach(batches, divL2, limit=4096):
    """the smallest number of Jacobi sweeps (searched over 1, 2, 3, 4, 6, 8, 12, 16 ... <= limit) whose projection reaches `divL2` on the
    held-out batches, or None"""
    n, step = 1, 1
    while n <= limit:
        if jacobi_divL2(batches, n) <= divL2:
            return n
        if n >= 4 * step:
            step *= 2
        n += step
    return None


def _hybrid_iterations(dim, net, batches, tol, max_iter):
    cold, warm = [], []
    with torch.no_grad():
        for data, _ in batches:
            flags, U = data[:, dim.iflags].contiguous(), data[:, dim.iU].contiguous()
            is3d = dim.nU == 3
            div = fluid.velocityDivergence(U, flags)
            p0, _ = net(data)
            cold += ext.solve_linear_system_pcg(flags, div, is3d, float(tol), int(max_iter), False, None)[2]
            warm += ext.solve_linear_system_pcg(flags, div, is3d, float(tol), int(max_iter), False, None, p0.contiguous())[2]
    return cold, warm


def hybrid_iterations(net, batches, tol=1e-5, max_iter=100):
    """what a trained net is worth to simulate(..., 'hybrid'): for each held-out batch [(data, target)] the CG iterations of
    solveLinearSystemPCG on div(U) to `tol` (> 0) from zero and from the net's pressure.  Returns (cold, warm), two lists with one count per sample in
    batch order.  2D and 3D batches alike (by the number of channels of `data`)."""
    assert tol > 0, "the iteration counts are those of a solve that stops at a tolerance"
    batches = list(batches)
    dim = _DIM
    if batches and batches[0][0].size(1) == 6:
        from .training3d import _DIM3 as dim
    return _hybrid_iterations(dim, net, batches, tol, max_iter)


def train(mconf=None, tconf=None, device="cuda", out=None, resume=None, log=None):
    """One training run.  mconf: the reference's modelParam keys (MCONF_DEFAULTS); tconf: TCONF_DEFAULTS (res or (H, W) via 'H', 'W';
    batch; iters; seed; sceneLength; stride; evalEvery; evalBatches; saveEvery).  `resume`: a checkpoint (path or dict) of a run with the
    same configuration -- the run continues from its iteration with the bits an uninterrupted run would have.  `out`: where the
    checkpoint {'state_dict', 'optimizer', 'mconf', 'it'} (+ 'scheduler', 'sampler', 'tconf', 'history' for the resume) is written at the
    end and every saveEvery iterations.  Returns dict(net, checkpoint, history); history rows are dict(it, loss, lt, lr[, val...])."""
    mconf = dict(MCONF_DEFAULTS, **(mconf or {}))
    tconf = dict(TCONF_DEFAULTS, **(tconf or {}))
    if mconf.get("is3D", False):
        raise ValueError("fluidnet_cxx_amd.training.train: training is 2D only (is3D=True)")
    _refuse_3d("train", tconf.get("D", 1))
    H, W = int(tconf.get("H", tconf["res"])), int(tconf.get("W", tconf["res"]))
    return _train(_DIM_BANK if mconf.get("model", "ScaleNet") == "FluidNet" else _DIM, mconf, tconf, (H, W), device, out, resume, log)
