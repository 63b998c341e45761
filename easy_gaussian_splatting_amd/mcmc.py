"""Training under a Gaussian budget: the densification of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al.,
2024) on the flat `optim.FusedAdam` buffers (csrc/gs_mcmc.hip; DESIGN.md, "Training to a budget").

    strategy = MCMCStrategy(model, cap_max=1_500_000)
    ...
    loss = render_loss + strategy.regularization()
    loss.backward(); optimizer.step(); optimizer.zero_grad()
    strategy.after_step(step)

or, inside the captured step (`train_graph.TrainStepGraph`; INTEGRATION.md "Training to a budget, captured"):

    strategy = MCMCStrategy(model, cap_max=1_500_000, noise="counter", seed=7)
    runner = TrainStepGraph(model, optimizer, loss_computer, data, gt, mcmc=strategy)
    ...
    runner.step(data, gt); strategy.after_step(step, runner)

Three parts: `relocate()` moves dead Gaussians (opacity <= min_opacity) onto live ones drawn in proportion to opacity, `grow()`
adds 5 % per refinement until the hard cap `cap_max`, `inject_noise()` perturbs the means after every optimizer step.  N is known
on the host at all times and stops changing at the cap; nothing reads the device to size anything.  `densify_and_prune` stays the
model's default refinement; this is the alternative for "train this scene with at most N Gaussians".

The seams (`opacity_weights`, `weight_cdf`, `sample_by_weight`, `relocation_values`) are the stages of the kernels as functions
that return tensors.  There is no torch or CPU path: HIP tensors only.

`noise="counter"`: the normals of Gaussian n at optimizer step t are a pure function of (seed, t, n) (Philox4x32-10 in the kernel,
`counter_normals` is the seam), drawn where they are applied -- no `torch.randn`, no z array, and a captured step the guard skipped
draws the same normals when the runner replays it.  In that mode the noise of a step comes BEFORE its relocate / grow (inside the
captured step it cannot come anywhere else), in the eager loop too, so that the two loops walk the same trajectory.

Out of scope: `distributed.ViewParallelStep` / `train_graph.ViewParallelGraphStep` (replicas would need broadcast draws), and
relocate / grow inside the graph.  No default of the package changes.
"""
from __future__ import annotations

import ctypes as ct
from typing import Any, Dict, Optional, Tuple

import torch
from torch import Tensor, nn

from .distributed import is_distributed


def _native():
    from . import _native as nat
    return nat, nat.lib()


def _on_device(*tensors: Tensor) -> torch.device:
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda:
            raise NotImplementedError("easy_gaussian_splatting_amd.mcmc runs on a HIP device only: there is no torch or CPU path")
        if t.device != dev:
            raise ValueError("tensors on different devices")
    return dev


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def opacity_weights(logit_opacities: Tensor, min_opacity: float, grow: bool = False) -> Tuple[Tensor, Tensor]:
    """(w, dead) of float32 logits [n]: o = sigmoid(l) in fp64, dead = (o <= min_opacity) as int32 0/1, w = 0 where dead and
    max(1, floor(o 2^24)) elsewhere, held in an int32 tensor (values <= 2^24).  `grow=True`: nothing is dead."""
    dev = _on_device(logit_opacities)
    nat, L = _native()
    l = logit_opacities.detach().reshape(-1)
    if l.dtype != torch.float32 or not l.is_contiguous():
        l = l.float().contiguous()
    n = l.numel()
    w = torch.empty((n,), dtype=torch.int32, device=dev)
    dead = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(L.gs_mcmc_weights(_stream(dev), n, l.data_ptr(), float(min_opacity), int(bool(grow)), w.data_ptr(), dead.data_ptr()),
                  "gs_mcmc_weights")
    return w, dead


def _as_weights(w: Tensor) -> Tensor:
    if w.dtype != torch.int32:
        raise TypeError("weights: an int32 tensor (opacity_weights)")
    return w.reshape(-1).contiguous()


def weight_cdf(w: Tensor) -> Tensor:
    """Inclusive prefix sum of the weights [n] as int64: exact, and the same whatever order the blocks run in."""
    dev = _on_device(w)
    nat, L = _native()
    w = _as_weights(w)
    n = w.numel()
    cdf = torch.empty((n,), dtype=torch.int64, device=dev)
    ws = torch.empty((int(L.gs_mcmc_cdf_workspace_longs(n)),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nat.check(L.gs_mcmc_cdf(_stream(dev), n, w.data_ptr(), cdf.data_ptr(), ws.data_ptr()), "gs_mcmc_cdf")
    return cdf


def _sample(w: Tensor, bits: Tensor, n_draws: Optional[int], dead: Optional[Tensor]) -> Dict[str, Tensor]:
    dev = _on_device(w, bits) if dead is None else _on_device(w, bits, dead)
    if (n_draws is None) == (dead is None):
        raise ValueError("give either dead (relocate: as many draws as dead Gaussians, counted on the device) or n_draws (grow)")
    if bits.dtype != torch.int64:
        raise TypeError("bits: an int64 tensor, 64 random bits per draw")
    nat, L = _native()
    w, bits = _as_weights(w), bits.reshape(-1).contiguous()
    n = w.numel()
    n_slots = n if dead is not None else int(n_draws)
    if n_slots < 0 or bits.numel() < n_slots:
        raise ValueError(f"bits holds {bits.numel()} words, {n_slots} are needed (relocate: one per Gaussian; grow: one per draw)")
    i32 = dict(dtype=torch.int32, device=dev)
    src, dst = torch.empty((n_slots,), **i32), torch.empty((n_slots,), **i32)
    counts, nd = torch.empty((n,), **i32), torch.empty((1,), dtype=torch.int64, device=dev)
    cdf = weight_cdf(w)
    st = _stream(dev)
    with torch.cuda.device(dev):
        if dead is not None:
            if dead.dtype != torch.int32 or dead.numel() != n:
                raise ValueError("dead: int32 [n] (opacity_weights)")
            dead = dead.reshape(-1).contiguous()
            incl = torch.empty_like(dead)
            scan_ws = torch.empty((int(L.gs_scan_rows_workspace_ints(1, n)),), **i32)
            nat.check(L.gs_scan_rows_i32(st, 1, n, dead.data_ptr(), incl.data_ptr(), scan_ws.data_ptr()), "gs_scan_rows_i32")
            nat.check(L.gs_mcmc_sample(st, n, n_slots, cdf.data_ptr(), bits.data_ptr(), dead.data_ptr(), incl.data_ptr(), 0,
                                       src.data_ptr(), dst.data_ptr(), counts.data_ptr(), nd.data_ptr()), "gs_mcmc_sample")
        else:
            nat.check(L.gs_mcmc_sample(st, n, n_slots, cdf.data_ptr(), bits.data_ptr(), None, None, n_slots,
                                       src.data_ptr(), dst.data_ptr(), counts.data_ptr(), nd.data_ptr()), "gs_mcmc_sample")
    return {"src": src, "dst": dst, "counts": counts, "n_draws": nd}


def sample_by_weight(w: Tensor, bits: Tensor, n_draws: Optional[int] = None, dead: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Draws Gaussians in proportion to the integer weights `w` [n].  `bits`: int64, 64 random bits per draw, read as uint64 b_j;
    draw j takes t_j = mulhi64(b_j, total) with total = sum(w) and src[j] = min{i : cdf[i] > t_j}.
    Relocate: `dead` (int32 0/1 [n]) -- as many draws as there are dead Gaussians, counted on the device; `bits` holds n words.
    Grow: `n_draws`, known on the host; `bits` holds n_draws words.  No draws when every weight is zero.
    Returns (src int32 [slots] with -1 beyond the draws, counts int32 [n], n_draws_dev int64 [1])."""
    r = _sample(w, bits, n_draws, dead)
    return r["src"], r["counts"], r["n_draws"]


def relocation_values(opacities: Tensor, scales: Tensor, ratio: Tensor) -> Tuple[Tensor, Tensor]:
    """Opacity and scales of a Gaussian that `ratio` copies replace (the paper's eq. 9), in fp64 from float32 inputs:
    R = clamp(ratio, 1, 51), o' = 1 - (1 - o)^(1/R), s' = s o / D, D = sum_{i=1..R} sum_{k<i} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1).
    opacities [n], scales [n, 3], ratio [n] integers; returns (o' [n], s' [n, 3]) as float32, unclamped."""
    dev = _on_device(opacities, scales, ratio)
    nat, L = _native()
    o = opacities.detach().reshape(-1).float().contiguous()
    n = o.numel()
    s = scales.detach().float().contiguous()
    if s.shape != (n, 3) or ratio.numel() != n:
        raise ValueError("opacities [n], scales [n, 3], ratio [n]")
    r = ratio.reshape(-1).to(torch.int32).contiguous()
    new_o, new_s = torch.empty_like(o), torch.empty_like(s)
    with torch.cuda.device(dev):
        nat.check(L.gs_mcmc_relocation_values(_stream(dev), n, o.data_ptr(), s.data_ptr(), r.data_ptr(), new_o.data_ptr(), new_s.data_ptr()),
                  "gs_mcmc_relocation_values")
    return new_o, new_s


def counter_normals(n: int, step: int, seed: int, device) -> Tensor:
    """float32 [n, 3]: the standard normals of Gaussians 0 .. n-1 at optimizer step `step` under the 64-bit `seed` -- one
    Philox4x32-10 block per Gaussian (counter: n and step, key: seed), Box-Muller in fp64, one rounding (include/gs_raster.h)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NotImplementedError("easy_gaussian_splatting_amd.mcmc runs on a HIP device only: there is no torch or CPU path")
    nat, L = _native()
    z = torch.empty((int(n), 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(L.gs_mcmc_normals(_stream(dev), int(n), int(step), int(seed) & _U64, z.data_ptr()), "gs_mcmc_normals")
    return z


_U64 = (1 << 64) - 1


class _BudgetReg(torch.autograd.Function):
    """a mean(sigmoid(logit)) + b mean(exp(log_scale)) through gs_mcmc_reg: the value in forward, the gradients in backward."""

    @staticmethod
    def forward(ctx, logit: Tensor, log_scales: Tensor, a: float, b: float) -> Tensor:
        dev = _on_device(logit, log_scales)
        nat, L = _native()
        n = logit.numel()
        if logit.dtype != torch.float32 or log_scales.dtype != torch.float32 or not logit.is_contiguous() or not log_scales.is_contiguous() \
                or log_scales.numel() != 3 * n:
            raise ValueError("regularization(fused=True): contiguous float32 logit_opacities [N] and log_scales [N, 3]")
        ws = torch.empty((int(L.gs_mcmc_reg_workspace_floats(n)),), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nat.check(L.gs_mcmc_reg(_stream(dev), n, logit.data_ptr(), log_scales.data_ptr(), a, b, None, ws.data_ptr(), None, None), "gs_mcmc_reg")
        ctx.save_for_backward(logit, log_scales)
        ctx.ab, ctx.ws = (a, b), ws
        return ws[0].clone()

    @staticmethod
    def backward(ctx, g: Tensor):
        logit, log_scales = ctx.saved_tensors
        nat, L = _native()
        dev, n = logit.device, logit.numel()
        v_l, v_s = torch.zeros_like(logit), torch.zeros_like(log_scales)
        with torch.cuda.device(dev):
            nat.check(L.gs_mcmc_reg(_stream(dev), n, logit.data_ptr(), log_scales.data_ptr(), ctx.ab[0], ctx.ab[1], None, ctx.ws.data_ptr(),
                                    v_l.data_ptr(), v_s.data_ptr()), "gs_mcmc_reg")
        return v_l * g, v_s * g, None, None


def random_bits(n: int, device, generator: Optional[torch.Generator] = None) -> Tensor:
    """n words of 64 random bits as int64 (two 32-bit draws each)."""
    hi = torch.randint(-2 ** 31, 2 ** 31, (n,), dtype=torch.int64, device=device, generator=generator)
    lo = torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, device=device, generator=generator)
    return (hi << 32) | lo


class MCMCStrategy:
    """Relocate / grow / noise around an eager train loop (module docstring).  The settings live here, not on the model: a
    checkpoint keeps holding only what the reference's classes can hold."""

    def __init__(self, model, cap_max: int, noise_lr: float = 5e5, refine_start: int = 500, refine_stop: int = 25_000,
                 refine_every: int = 100, min_opacity: float = 0.005, grow_factor: float = 1.05,
                 generator: Optional[torch.Generator] = None, noise: str = "torch", seed: int = 0):
        """`noise`: "torch" (default) -- `inject_noise` draws `torch.randn` from `generator`; "counter" -- the draws are a pure function
        of (`seed`, step, Gaussian), made in the kernel: the form `TrainStepGraph(mcmc=...)` needs (module docstring)."""
        from .optim import FusedAdam
        if noise not in ("torch", "counter"):
            raise ValueError("noise: 'torch' or 'counter'")
        self.noise, self.seed = noise, int(seed) & _U64
        self._rec: Optional[Tensor] = None
        if is_distributed():
            raise NotImplementedError("MCMCStrategy under torch.distributed: the replicas would need broadcast draws")
        if int(cap_max) < model.nbr_gaussians:
            raise ValueError(f"cap_max = {cap_max} is below the model's {model.nbr_gaussians} Gaussians")
        if not isinstance(model.optimizer, FusedAdam) or not model.means.is_cuda:
            raise NotImplementedError("MCMCStrategy works in place on optim.FusedAdam's flat buffers on a HIP device "
                                      "(build_optimizers(..., fused='hip') on a GPU model); there is no torch or CPU path")
        if not 0.0 <= float(min_opacity) < 1.0 or float(grow_factor) < 1.0 or int(refine_every) < 1:
            raise ValueError("0 <= min_opacity < 1, grow_factor >= 1, refine_every >= 1")
        self.model, self.cap_max, self.noise_lr = model, int(cap_max), float(noise_lr)
        self.refine_start, self.refine_stop, self.refine_every = int(refine_start), int(refine_stop), int(refine_every)
        self.min_opacity, self.grow_factor, self.generator = float(min_opacity), float(grow_factor), generator

    # ---- the loss term
    def regularization(self, opacity_reg: float = 0.01, scale_reg: float = 0.01, fused: bool = False) -> Tensor:
        """opacity_reg mean(opacities) + scale_reg mean(scales): what makes unused Gaussians die so that relocation can move them.
        `fused=True`: one HIP pass over the raw logits and log-scales (gs_mcmc_reg) for the value and one for the gradients --
        the arithmetic of the captured step's term, bit for bit."""
        if fused:
            return _BudgetReg.apply(self.model.logit_opacities, self.model.log_scales, float(opacity_reg), float(scale_reg))
        return opacity_reg * self.model.opacities.mean() + scale_reg * self.model.scales.mean()

    # ---- plumbing
    def _widths(self):
        return [3, 3, 4, 3, 3 * self.model.sh_rest.shape[1], 1]

    def _apply(self, n: int, n_rows: int, r: Dict[str, Tensor], max_draws: int, p: Tensor, m: Tensor, v: Tensor, offs) -> None:
        nat, L = _native()
        dev = p.device
        K = 1 + self.model.sh_rest.shape[1]
        with torch.cuda.device(dev):
            nat.check(L.gs_mcmc_apply(_stream(dev), n, n_rows, K, self.min_opacity, r["src"].data_ptr(), r["dst"].data_ptr(),
                                      r["counts"].data_ptr(), r["n_draws"].data_ptr(), max_draws, p.data_ptr(), m.data_ptr(), v.data_ptr(),
                                      (ct.c_int64 * 6)(*offs)), "gs_mcmc_apply")

    # ---- the three parts
    @torch.no_grad()
    def relocate(self) -> Dict[str, Tensor]:
        """Dead Gaussians take the parameters of live ones drawn in proportion to opacity; the drawn ones share their opacity and
        scale out over their copies.  In place, N unchanged, no host read: the returned device tensors (`n_dead` int64 [1], `src`,
        `dst`, `counts`) cost a synchronisation only when the caller looks at them."""
        model, opt = self.model, self.model.optimizer
        opt._check_views()
        n, dev = model.nbr_gaussians, model.means.device
        w, dead = opacity_weights(model.logit_opacities, self.min_opacity)
        r = _sample(w, random_bits(n, dev, self.generator), None, dead)
        self._apply(n, n, r, n, opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt._offs)
        return {"n_dead": r["n_draws"], "src": r["src"], "dst": r["dst"], "counts": r["counts"]}

    @torch.no_grad()
    def grow(self) -> int:
        """Adds min(cap_max, int(grow_factor N)) - N Gaussians, each a copy of one drawn in proportion to opacity (values shared
        out as in `relocate`), in fresh flat buffers the optimizer adopts.  Returns the number added; 0 at the cap."""
        from .optim import FusedAdam
        model, opt = self.model, self.model.optimizer
        opt._check_views()
        n, dev = model.nbr_gaussians, model.means.device
        n_new = max(0, min(self.cap_max, int(self.grow_factor * n)) - n)
        if n_new == 0:
            return 0
        n_tot, widths, K = n + n_new, self._widths(), 1 + model.sh_rest.shape[1]
        old_offs = list(opt._offs)
        new_offs, _, total = FusedAdam.flat_layout([n_tot * wd for wd in widths])
        f32 = dict(dtype=torch.float32, device=dev)
        new_p, new_m, new_v = torch.zeros(total, **f32), torch.zeros(total, **f32), torch.zeros(total, **f32)   # (pads and new moments: zero)
        for old, new in ((opt.flat_param, new_p), (opt.exp_avg, new_m), (opt.exp_avg_sq, new_v)):
            for oo, no, wd in zip(old_offs, new_offs, widths):
                new[no:no + n * wd].copy_(old[oo:oo + n * wd])
        w, _ = opacity_weights(model.logit_opacities, self.min_opacity, grow=True)
        r = _sample(w, random_bits(n_new, dev, self.generator), n_new, None)
        self._apply(n, n_tot, r, n_new, new_p, new_m, new_v, new_offs)
        shapes = {"means": (n_tot, 3), "log_scales": (n_tot, 3), "quats": (n_tot, 4), "sh_0": (n_tot, 1, 3),
                  "sh_rest": (n_tot, K - 1, 3), "logit_opacities": (n_tot,)}
        new_params = []
        for name, o, wd in zip(model.param_names, new_offs, widths):
            setattr(model, name, nn.Parameter(new_p[o:o + n_tot * wd].view(shapes[name])))
            new_params.append(getattr(model, name))
        opt.adopt_flat(new_p, new_m, new_v, new_params)
        model.grad_norm_accum = torch.zeros((n_tot,), device=dev)
        model.collecting_counts = torch.zeros((n_tot,), device=dev)
        model.max_radii = torch.zeros((n_tot,), device=dev)
        return n_new

    @torch.no_grad()
    def inject_noise(self, means_lr: float, step: Optional[int] = None) -> None:
        """means += noise_lr means_lr g(o) Sigma z with z standard normal, Sigma = R diag(s^2) R^T and g a sharp gate that is
        1 for transparent Gaussians and 0 for opaque ones (1 / (1 + exp(-100 ((1 - o) - 0.995)))).  `noise="counter"`: z is the
        draw of (seed, `step`, Gaussian), made inside the kernel (gs_mcmc_step_inputs + gs_mcmc_noise_step)."""
        nat, L = _native()
        model = self.model
        model.optimizer._check_views()
        n, dev = model.nbr_gaussians, model.means.device
        if self.noise == "counter":
            if step is None:
                raise ValueError("inject_noise: noise='counter' draws per optimizer step, pass `step`")
            if self._rec is None or self._rec.device != dev:
                self._rec = torch.zeros((nat.GS_MCMC_REC_WORDS,), dtype=torch.int64, device=dev)
            # (every argument is formed first, so that the two launches reach the queue back to back)
            rec, strength = self._rec.data_ptr(), self.noise_lr * float(means_lr)
            ptrs = (model.log_scales.data_ptr(), model.quats.data_ptr(), model.logit_opacities.data_ptr(), model.means.data_ptr())
            with torch.cuda.device(dev):
                st = _stream(dev)
                rc0 = L.gs_mcmc_step_inputs(st, strength, int(step), self.seed, rec)
                rc1 = L.gs_mcmc_noise_step(st, n, rec, *ptrs)
            nat.check(rc0, "gs_mcmc_step_inputs")
            nat.check(rc1, "gs_mcmc_noise_step")
            return
        z = torch.randn((n, 3), device=dev, generator=self.generator)
        with torch.cuda.device(dev):
            nat.check(L.gs_mcmc_noise(_stream(dev), n, self.noise_lr * float(means_lr), model.log_scales.data_ptr(), model.quats.data_ptr(),
                                      model.logit_opacities.data_ptr(), z.data_ptr(), model.means.data_ptr()), "gs_mcmc_noise")

    def _means_lr(self) -> float:
        for group in self.model.optimizer.param_groups:
            if group.get("name") == "means":
                return float(group["lr"])
        raise RuntimeError("the param_group 'means' isn't in the optimizer")

    def after_step(self, step: int, runner=None) -> Dict[str, Any]:
        """To be called after `optimizer.step()`: relocate + grow every `refine_every` steps inside (refine_start, refine_stop],
        noise always, at the current learning rate of the optimizer's `means` group.
        `runner` (a `TrainStepGraph(mcmc=self)`, to be called after its `step()`): the noise ran inside the step; before rows move
        the runner's pending steps are applied (`finish()`: one block per `refine_every` steps).  `relocate()` works in place and the
        graph is kept; `grow()` changes N and the storage, which the runner answers with a re-build on its next `step()`."""
        info: Dict[str, Any] = {}
        refine = self.refine_start < step <= self.refine_stop and step % self.refine_every == 0
        if runner is not None:
            if getattr(runner, "mcmc", None) is not self:
                raise ValueError("after_step(step, runner): the runner was not built with mcmc=<this strategy>")
            if refine:
                runner.finish()
        elif self.noise == "counter":   # in front of relocate / grow, where the captured step has it
            self.inject_noise(self._means_lr(), step)
        if refine:
            info["relocate"] = self.relocate()
            info["n_new"] = self.grow()
        if runner is None and self.noise == "torch":
            self.inject_noise(self._means_lr())
        return info
