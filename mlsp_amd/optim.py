"""Adam over ONE flat parameter buffer: the optimizer step of the hot path as a single launch.

PointDA/trainer.py:258-259 builds `optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.wd)`.  torch's fused Adam walks the 77
parameter tensors of DGCNN + heads in 64 Ki-element chunks, one chunk per workgroup: most tensors end in a mostly empty chunk, five to
six launches per step, 110 us at 1.2 TB/s for 127 MB of parameter / gradient / moment traffic (profiles/r5_*).  Here the parameters and
both moments live in three flat fp32 buffers (the parameters become views), the gradients autograd produced are read where they lie through a
pointer table, and ONE launch of `mlsp_adam_flat_groups_f32` (csrc/optim.hip: 2048-element tiles, ~2300 workgroups, the element-wise update of
torch's fused kernel restated type by type and lowering by lowering) steps every parameter that holds a gradient: 19 us.
tests/test_gpu_optim.py asserts bit-identity with `torch.optim.Adam(..., fused=True)` on the unflattened model step by step.
(torch's own fused kernel on the same flat buffers, as one tensor, measured 88 us: its chunking is per 64 Ki elements whatever the
tensor list looks like.)

Layout.  Parameters that already SHARE a storage keep their relative places: the merged head layers make the parameters they read as one
operand adjacent in one buffer (functional.rehome_adjacent), and moving them apart again would cost a concatenation per forward.  Every such
storage -- and every stand-alone parameter -- becomes one unit, placed on a 256-byte boundary (an arbitrary offset into a flat buffer would
send every GEMM that reads the weight to its unaligned edge-tile instantiation: 4.48 -> 6.10 ms per step measured).  If parameters leave the
buffer later (module.to(), another rehome_adjacent) the layout is rebuilt at the next step, moments and step counter carried over.

Semantics kept from torch: a parameter whose gradient is None is not stepped (DGCNN.Rec_scan in the default modes, Models.py:150) and gets
no state; every group's `lr` and other options are read from `param_groups` at every step (CosineAnnealingLR, trainer.py:260);
`state_dict()` / `load_state_dict()` see per-parameter `step` / `exp_avg` / `exp_avg_sq` entries (views of the flat moments).

Parameter groups (up to 8: "no weight decay on BatchNorm and biases" -- the reference's utils/optimizer.py:18-36 add_weight_decay --,
per-group learning rates).  The trainable parameters of ALL groups live in the one flat buffer, laid out by storage unit in address order
as above; a group is a TAG on a segment, not a region: parameters that share a storage stay adjacent although a merged weight is decayed
and the bias next to it is not.  The launch carries one byte per segment and a table of the groups' hyperparameters
(`mlsp_adam_flat_groups_f32`); a workgroup reads the entry of the segment that owns its tile.  Adam keeps one device-side step counter per
GROUP (torch: per parameter): loaded state whose groups are at different steps is fine, two step counts inside one group are not.  A group
none of whose parameters ever holds a gradient has no segments and no state.  `add_param_group` after the first step lays everything out
again at the next step -- the state that exists carried over, the new group's counter at 0.  AdamW: `decoupled_weight_decay=True` in a
group (torch.optim.Adam's flag), or FlatAdamW, a torch.optim.AdamW subclass; bit-identical to torch.optim.AdamW(fused=True)
(tests/test_gpu_optim_groups.py).

The flat step needs fp32 parameters on one device and the SAME set of parameters holding gradients at every step (a group's parameters
share its step counter); anything else -- more than 8 groups, a group with amsgrad / maximize / capturable / differentiable / a tensor
lr / fused=False, a parameter set that changes between steps -- falls back to torch's own per-tensor path for good, on the same storage,
with the state carried over.

FlatSGD does the same for torch.optim.SGD (the trainers' `--optimizer SGD`): parameters and momentum buffer in flat buffers, ONE launch of
`mlsp_sgd_flat_groups_f32`, bit-identical to torch's default multi-tensor SGD (tests/test_gpu_optim_sgd.py).  The layout, the fixed set of stepped
parameters, the rebuild, the hand-over to torch and the published weight bounds are one piece of code for both (_FlatStep).
"""
import ctypes

import torch

from . import _lib


def flat_offsets(params, align=1):
    """(first element of every parameter, total elements) of a flat buffer that holds `params` back to back, each starting on a multiple
    of `align` elements (FlatGradSync's bucket layout)."""
    offs, n = [], 0
    for p in params:
        n = (n + align - 1) // align * align
        offs.append(n)
        n += p.numel()
    return offs, (n + align - 1) // align * align


def storage_unit_offsets(params, align):
    """Offsets for `params` in a flat buffer in which parameters that share a storage keep their relative byte offsets (one unit per
    shared storage, spanning its members; stand-alone parameters are units of their own), every unit starting on a multiple of `align`
    elements.  -> (offsets in elements, total elements), or None when some parameter is not a dense contiguous fp32 tensor."""
    units, order = {}, []
    for i, p in enumerate(params):
        if not p.is_contiguous() or p.dtype != torch.float32:
            return None
        key = p.untyped_storage().data_ptr()
        if key not in units:
            units[key] = []
            order.append(key)
        units[key].append(i)
    offs, n = [0] * len(params), 0
    for key in order:
        members = units[key]
        lo = min(params[i].data_ptr() for i in members)
        hi = max(params[i].data_ptr() + 4 * params[i].numel() for i in members)
        if len(members) == 1 or (hi - lo) // 4 > 8 * sum(params[i].numel() for i in members):
            # a lone parameter -- or members scattered over a big foreign storage (views of something else; span > 8x the content,
            # both in elements): place them one by one
            for i in members:
                n = (n + align - 1) // align * align
                offs[i] = n
                n += params[i].numel()
            continue
        n = (n + align - 1) // align * align
        for i in members:
            d = params[i].data_ptr() - lo
            if d % 4:
                return None
            offs[i] = n + d // 4
        n += (hi - lo) // 4
    # the members of a unit are distinct parameters of one concatenation: they must not overlap
    spans = sorted((offs[i], offs[i] + p.numel()) for i, p in enumerate(params))
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        return None
    return offs, (n + align - 1) // align * align


def _on_gpu(params):
    """whether an optimizer's `params` argument (tensors or group dicts) holds GPU tensors"""
    return any(isinstance(p, torch.Tensor) and p.is_cuda for p in params) or any(
        isinstance(g, dict) and any(p.is_cuda for p in g["params"]) for g in params)


class _FlatStep:
    """The flat-buffer machinery FlatAdam and FlatSGD share (mixed in front of their torch optimizer): the storage-unit layout, the fixed
    set of parameters that step, the rebuild when parameters left the buffer, the hand-over to torch's own path for good, and the tile
    maxima the step kernel leaves (weight_bounds).  A subclass supplies

      _group_ok(g)                     whether the flat step covers the options of parameter group g
      _state_fits(ps, gid, active)     whether the existing optimizer state can move into flat buffers
      _adopt_state(ps, gid, active, offs, n, dev) -> dict    its flat state buffers (existing state copied in), merged into the layout
      _flat_fits(f)                    whether a built layout still serves the current options (else: torch's path from now on)
      _launch(f, groups, grads, n)     the one launch (groups: self.param_groups, read at every step; grads: ctypes array of n gradient
                                       pointers, in the order of the active segments; f["seg_group"]: the group of every segment)
      _LEAVE_MSG                       the warning when the one-launch step is given up ("%s": why)

    ps is the list of trainable parameters of ALL groups, group after group; gid[i] is the group of ps[i].  The groups are tags on the
    segments, not regions of the buffer: the layout orders storage units by address whatever group their members belong to.
    """
    ALIGN = 64
    MAX_GROUPS = _lib.FLAT_MAX_GROUPS

    def _flat_init(self):
        self._flat = None              # the flat buffers and their layout once built (dict)
        self._active = None            # indices (into the trainable parameter list) of the parameters that step, fixed at the first step
        self._disabled = False         # True: torch's per-tensor path from now on
        self.flat_steps = 0            # steps taken on the flat path (tests)
        self.layouts_built = 0         # (tests: a rebuild happens only when parameters left the buffer or a group was added)
        self._regroup = False          # a parameter group was added since the layout was built

    def _flat_params_ok(self):
        """dense fp32 parameters on one GPU.  Asked before a layout is built or rebuilt, not at every step: while a layout stands, the
        step verifies that every parameter still lies at its place in the flat fp32 buffer, which says the same."""
        dev = None
        for g in self.param_groups:
            for p in g["params"]:
                if dev is None:
                    dev = p.device
                if not (p.dtype == torch.float32 and p.device == dev and p.is_cuda and not p.is_sparse):
                    return False
        return dev is not None

    def _eligible(self):
        """whether this step can be a flat one: at most MAX_GROUPS groups, each with options the flat step covers (read at every step:
        anybody may write param_groups), and -- before a layout exists -- parameters it can hold"""
        groups = self.param_groups
        if self._disabled or not 1 <= len(groups) <= self.MAX_GROUPS:
            return False
        for g in groups:
            if not self._group_ok(g):
                return False
        return self._flat is not None or self._flat_params_ok()

    def _state_fits(self, ps, gid, active):
        return True

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if getattr(self, "_flat", None) is not None:
            # lay everything out again at the next step, around the parameters that hold gradients then: the state that exists is
            # carried over, the new group starts without any
            self._regroup = True

    def _flat_fits(self, f):
        return True

    def _on_leave(self, f):
        pass

    def _build(self):
        """Lay the trainable parameters out (storage units, see the module docstring), move them and whatever optimizer state exists into
        fresh flat buffers.  None: the existing state does not fit the flat step."""
        ps, gid = [], []
        for g, grp in enumerate(self.param_groups):
            for p in grp["params"]:
                if p.requires_grad:
                    ps.append(p)
                    gid.append(g)
        dev = ps[0].device
        lay = storage_unit_offsets(ps, self.ALIGN)
        if lay is None:
            lay = flat_offsets(ps, self.ALIGN)
        offs, n = lay
        active = self._active if self._active is not None else [i for i, p in enumerate(ps) if p.grad is not None]
        # (segments -- and with them the step kernel's tiles -- in ADDRESS order: parameters that one GEMM reads as a single operand, adjacent
        # in the buffer but not in model.parameters(), then own one contiguous run of tile maxima: weight_bounds)
        active = sorted(active, key=lambda i: offs[i])
        if not active or not self._state_fits(ps, gid, active):
            return None
        flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        views = [flat_p[o:o + p.numel()].view_as(p) for o, p in zip(offs, ps)]
        torch._foreach_copy_(views, [p.data for p in ps])
        for p, v in zip(ps, views):
            p.data = v                                    # the model now lives in the flat buffer (load_state_dict copies into it)
        extra = self._adopt_state(ps, gid, active, offs, n, dev)
        self._active = active
        self._regroup = False
        self.layouts_built += 1
        n_act = len(active)
        seg = ((ctypes.c_uint32 * n_act)(*[offs[i] for i in active]), (ctypes.c_uint32 * n_act)(*[ps[i].numel() for i in active]))
        # per-tile maxima of the updated parameters (csrc/optim.hip tile_amax): tiles run segment by segment in the order of `active`
        tile_begin, t = [], 0
        for i in active:
            tile_begin.append(t)
            t += (ps[i].numel() + 2047) // 2048
        tile_begin.append(t)
        f = {"params": ps, "gid": gid, "offs": offs, "p": flat_p, "seg": seg, "seg_group": (ctypes.c_uint8 * n_act)(*[gid[i] for i in active]),
             "tile_amax": torch.zeros(t, dtype=torch.float32, device=dev),
             "tile_begin": tile_begin, "amax_versions": None, "amax_map": {}}
        f.update(extra)
        return f

    def _leave_flat(self, why=None):
        """torch's own path from now on (same storage, the state carried over).  `why`: warn once -- the results are the same, the
        one-launch step is lost."""
        if why and not self._disabled:
            import warnings
            warnings.warn(self._LEAVE_MSG % why, RuntimeWarning, stacklevel=3)
        if self._flat is not None:
            self._on_leave(self._flat)
        self._flat, self._disabled = None, True

    # ---- the step -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._eligible() or (self._flat is not None and not self._flat_fits(self._flat)):
            if self._flat is not None:
                self._leave_flat("the parameter groups / options are no longer the ones the flat step covers")
            super().step()
            return loss
        if self._regroup:                                 # add_param_group since the last step: the parameters that step are chosen anew
            old_active, self._regroup, self._active = self._active, False, None
            f = self._build() if self._flat_params_ok() else None
            if f is None:
                self._active = old_active
                self._leave_flat("after add_param_group the parameters / the optimizer state no longer fit the flat step")
                super().step()
                return loss
            self._flat = f
        if self._flat is None:
            self._flat = self._build()
            if self._flat is None:
                self._leave_flat("the loaded optimizer state does not fit the flat step, or no parameter holds a gradient")
                super().step()
                return loss
        f = self._flat
        ps, act = f["params"], self._active
        n_with = sum(1 for p in ps if p.grad is not None)
        if n_with != len(act) or any(ps[i].grad is None for i in act):
            # another set of parameters holds gradients this step (a head that runs only in some steps): per-tensor semantics
            self._leave_flat("the set of parameters holding gradients changed between steps")
            super().step()
            return loss
        base, offs = f["p"].data_ptr(), f["offs"]
        if any(p.data_ptr() != base + 4 * offs[i] for i, p in enumerate(ps)):
            # parameters left the buffer (module.to(), a rehome_adjacent of a head that ran for the first time): lay them out again
            # around their new storages, optimizer state carried over
            f = self._build() if self._flat_params_ok() else None
            if f is None:
                self._leave_flat("parameters left the flat buffer and they, or the optimizer state, no longer fit the flat step")
                super().step()
                return loss
            self._flat = f
            ps, act = f["params"], self._active            # (the rebuild orders the segments by their NEW addresses)
        # one launch; every gradient is read where autograd (or the exchange's bucket) left it
        grads = [ps[i].grad if ps[i].grad.is_contiguous() else ps[i].grad.contiguous() for i in act]
        n = len(act)
        gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
        self._launch(f, self.param_groups, gp, n)
        # the kernel left the magnitude of every updated parameter tile: valid for as long as nobody else writes the parameters (an
        # in-place torch operation bumps the tensor's version counter -- the raw update above does not)
        f["amax_versions"] = [ps[i]._version for i in act]
        _lib.weight_bound_providers.add(self)
        self.flat_steps += 1
        return loss

    def invalidate_bounds(self):
        """Forget the parameter magnitudes the last step left (call after writing parameters in a way torch's version counters do not
        see: in-place operations on `.data`); the GEMMs measure their weights again until the next step."""
        if self._flat is not None:
            self._flat["amax_versions"] = None

    def weight_bounds(self, W):
        """(device pointer, n) of ready-made partial maxima bounding |W| for a GEMM operand W that lies inside the flat parameter buffer --
        the tiles of the parameters it overlaps, as the last step's kernel left them -- or None (not in the buffer, a parameter without
        a gradient in between, or written by someone else since the step: the caller measures)."""
        f = self._flat
        if f is None or f.get("amax_versions") is None or W.dim() != 2 or W.dtype != torch.float32 or W.stride(1) != 1:
            return None
        base, nbytes = f["p"].data_ptr(), f["p"].numel() * 4
        a = W.data_ptr() - base
        if a < 0 or a >= nbytes or a % 4:
            return None
        key = (a, W.shape[0], W.shape[1], W.stride(0))
        hit = f["amax_map"].get(key)
        if hit is None:
            a //= 4
            b = a + (W.shape[0] - 1) * W.stride(0) + W.shape[1]            # one past the last element W touches
            ps, offs, act = f["params"], f["offs"], self._active
            cover = [j for j, i in enumerate(act) if offs[i] < b and offs[i] + ps[i].numel() > a]
            ok = bool(cover) and cover == list(range(cover[0], cover[-1] + 1)) and a >= offs[act[cover[0]]] and b <= offs[act[cover[-1]]] + ps[act[cover[-1]]].numel()
            # (every element of W must lie inside some ACTIVE parameter: alignment gaps between units hold zeros, which is fine, but a
            # parameter that is not stepped has no tile)
            if ok:
                spans = sorted((offs[act[j]], offs[act[j]] + ps[act[j]].numel()) for j in cover)
                inactive = [(offs[i], offs[i] + p.numel()) for i, p in enumerate(ps) if i not in set(act)]
                ok = not any(lo < b and hi > a for lo, hi in inactive)
            hit = f["amax_map"][key] = (cover[0], cover[-1]) if ok else False
        if hit is False:
            return None
        j0, j1 = hit
        ps, act, ver = f["params"], self._active, f["amax_versions"]
        if any(ps[act[j]]._version != ver[j] for j in range(j0, j1 + 1)):
            return None
        t0, t1 = f["tile_begin"][j0], f["tile_begin"][j1 + 1]
        if t1 - t0 > 4096:
            return None
        return f["tile_amax"].data_ptr() + 4 * t0, t1 - t0

    def load_state_dict(self, state_dict):
        # loaded state holds fresh tensors: rebuild the flat buffers from them at the next step (parameters stay where they are)
        if self._flat is not None:
            self._leave_flat()
            self._disabled = False
        super().load_state_dict(state_dict)
        self._flat = None
        self._active = None
        self._regroup = False


def _per_group(gid, active, ngroups):
    """the active parameter indices of every group"""
    out = [[] for _ in range(ngroups)]
    for i in active:
        out[gid[i]].append(i)
    return out


class FlatAdam(_FlatStep, torch.optim.Adam):
    """torch.optim.Adam over flat buffers (module docstring).  `decoupled_weight_decay=True` is AdamW's decay, as in torch.optim.Adam;
    every parameter group brings its own lr / betas / eps / weight_decay / decoupled_weight_decay and its own step counter.
    `state_dict()` hands out a `step` tensor of its own per parameter (a small device copy each), as torch.optim.Adam keeps them, so
    that the state loads into torch's optimizers; inside, a group's parameters share one counter."""
    _LEAVE_MSG = ("FlatAdam: leaving the one-launch flat step for torch's per-tensor fused Adam (%s); same results, but the "
                  "optimizer step takes ~5 launches / ~0.1 ms instead of 1 / ~0.02 ms from now on")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        params = list(params)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=_on_gpu(params),
                         decoupled_weight_decay=decoupled_weight_decay)
        self._flat_init()

    def _group_ok(self, g):
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable") or not g.get("fused"):
            return False
        return not any(isinstance(v, torch.Tensor) for v in (g["lr"], g["eps"], g["weight_decay"], *g["betas"]))

    def _state_of(self, ps, gid, active):
        """per group: (the step counts its active parameters are at, those of them that have moments)"""
        out = []
        for members in _per_group(gid, active, len(self.param_groups)):
            steps = {float(self.state[ps[i]]["step"]) for i in members if ps[i] in self.state and "step" in self.state[ps[i]]}
            have = {i for i in members if ps[i] in self.state and "exp_avg" in self.state[ps[i]]}
            out.append((members, steps, have))
        return out

    def _state_fits(self, ps, gid, active):
        """per group one shared step counter and moments for every active parameter or none; no state elsewhere"""
        act = set(active)
        if any(p in self.state and self.state[p] for i, p in enumerate(ps) if i not in act):
            return False
        return not any(len(steps) > 1 or (have and len(have) != len(members)) for members, steps, have in self._state_of(ps, gid, active))

    def _adopt_state(self, ps, gid, active, offs, n, dev):
        flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        groups = self._state_of(ps, gid, active)
        host_steps = [int(round(steps.pop())) if steps else 0 for _, steps, _ in groups]
        # one device-side counter per group, shared by the group's parameters (their state["step"] is a 0-dim view of it)
        steps = torch.tensor([float(h) for h in host_steps], dtype=torch.float32, device=dev)
        for g, (members, _, have) in enumerate(groups):
            for i in members:
                p, o = ps[i], offs[i]
                m, v = flat_m[o:o + p.numel()].view_as(p), flat_v[o:o + p.numel()].view_as(p)
                if i in have:
                    m.copy_(self.state[p]["exp_avg"])
                    v.copy_(self.state[p]["exp_avg_sq"])
                self.state[p] = {"step": steps[g], "exp_avg": m, "exp_avg_sq": v}
        table = (_lib.MlspAdamGroup * len(groups))()
        for g, (members, _, _) in enumerate(groups):
            table[g].step_out = steps[g].data_ptr() if members else None      # (a group none of whose parameters steps has no counter ...)
            table[g].step = 1                                                  # (... and its entry a step number nobody reads)
        return {"m": flat_m, "v": flat_v, "step": steps, "host_step": host_steps, "stepping": [bool(m) for m, _, _ in groups], "table": table,
                "seen": [None] * len(groups)}

    def _flat_fits(self, f):
        return len(self.param_groups) == len(f["table"]) or self._regroup

    def state_dict(self):
        # (a group's parameters share one counter tensor here; what leaves gets a counter per parameter, as torch.optim.Adam keeps them:
        # loaded into torch's optimizer, a shared tensor would be incremented once per parameter)
        sd = super().state_dict()
        sd["state"] = {k: ({**v, "step": v["step"].clone()} if torch.is_tensor(v.get("step")) else v) for k, v in sd["state"].items()}
        return sd

    def _on_leave(self, f):
        # every stepped parameter gets its own step counter
        for i in self._active:
            st = self.state[f["params"][i]]
            st["step"] = st["step"].clone()

    def _launch(self, f, groups, gp, n):
        table, hs, seen, stepping = f["table"], f["host_step"], f["seen"], f["stepping"]
        for g, grp in enumerate(groups):
            t = table[g]
            opts = (grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"], grp.get("decoupled_weight_decay"))
            if opts != seen[g]:                           # (an entry is rewritten only when the group's options moved: a scheduler's lr)
                seen[g] = opts
                t.lr, t.eps, t.weight_decay = float(opts[0]), float(opts[2]), float(opts[3])
                t.beta1, t.beta2 = float(opts[1][0]), float(opts[1][1])
                t.decoupled = int(bool(opts[4]))
            if stepping[g]:
                hs[g] += 1
                t.step = hs[g]
        _lib.check(_lib.load().mlsp_adam_flat_groups_f32(f["p"].data_ptr(), f["m"].data_ptr(), f["v"].data_ptr(), f["seg"][0], f["seg"][1], gp,
                                                         f["seg_group"], n, table, len(table), f["tile_amax"].data_ptr(), _lib.stream()),
                   "mlsp_adam_flat_groups_f32")


class FlatAdamW(FlatAdam, torch.optim.AdamW):
    """torch.optim.AdamW (decoupled weight decay, default 1e-2) on FlatAdam's one-launch step: the trainers' "AdamW, no decay on BatchNorm
    and biases" (the reference's utils/optimizer.py add_weight_decay: two parameter groups) stays one launch and keeps publishing weight
    bounds.  torch.optim.AdamW's constructor defaults and validation; `state_dict()` is interchangeable with torch.optim.AdamW's; bit-
    identical to torch.optim.AdamW(fused=True) (tests/test_gpu_optim_groups.py)."""
    _LEAVE_MSG = FlatAdam._LEAVE_MSG.replace("FlatAdam", "FlatAdamW").replace("fused Adam", "fused AdamW")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        params = list(params)
        # (fused where the flat step can run; torch's own default on CPU parameters, where this class IS torch.optim.AdamW)
        torch.optim.AdamW.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=True if _on_gpu(params) else None)
        self._flat_init()


class FlatSGD(_FlatStep, torch.optim.SGD):
    """torch.optim.SGD (the trainers' `--optimizer SGD`: PointDA/trainer.py:258-259, PointDA/train_spst.py, PointSegDA/trainer.py:212-214)
    over one flat parameter buffer and one flat momentum buffer: ONE launch of `mlsp_sgd_flat_groups_f32` per step, bit-identical to torch's
    default (multi-tensor) SGD on GPU tensors.  Same constructor arguments and validation as torch.optim.SGD; per-parameter
    `momentum_buffer` entries are views of the flat buffer, and with momentum == 0 there is no state at all.  The step kernel leaves the
    per-tile magnitude bounds of the updated parameters as FlatAdam's does (weight_bounds).  The flat step needs what FlatAdam's needs
    (at most 8 groups of fp32 parameters on one GPU, the same set of parameters holding gradients at every step) and torch's default path
    (foreach, not fused or differentiable, float lr / momentum / weight_decay); anything else -- or loaded state in which only some
    stepped parameters have a momentum buffer -- falls back to torch's own path for good, with the state carried over.  Unlike torch's
    foreach path with nesterov and no weight decay, the gradients are left as autograd made them."""
    _LEAVE_MSG = ("FlatSGD: leaving the one-launch flat step for torch's multi-tensor SGD (%s); same results, but the optimizer step "
                  "takes several foreach launches from now on")

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        self._flat_init()

    def _group_ok(self, g):
        if g.get("differentiable") or g.get("fused") or g.get("foreach") is False:
            return False
        if any(isinstance(g[k], torch.Tensor) for k in ("lr", "momentum", "dampening", "weight_decay")):
            return False
        return not any(p.grad is not None and p.grad.is_sparse for p in g["params"])

    def _momentum_state(self, ps, gid, active):
        """per group with momentum: (its active parameters, those of them that have a momentum buffer); None for a group without"""
        return [(members, [i for i in members if "momentum_buffer" in self.state.get(ps[i], {})]) if grp["momentum"] != 0 else None
                for grp, members in zip(self.param_groups, _per_group(gid, active, len(self.param_groups)))]

    def _state_fits(self, ps, gid, active):
        """per group: momentum buffers for every active parameter or for none (torch would step the others per tensor)"""
        return all(ms is None or not ms[1] or len(ms[1]) == len(ms[0]) for ms in self._momentum_state(ps, gid, active))

    def _adopt_state(self, ps, gid, active, offs, n, dev):
        mstate = self._momentum_state(ps, gid, active)
        mom_on = [grp["momentum"] != 0 for grp in self.param_groups]
        table = (_lib.MlspSgdGroup * len(mstate))()
        if not any(mom_on):
            return {"b": None, "first": [False] * len(mstate), "mom_on": mom_on, "table": table, "seen": [None] * len(mstate)}
        flat_b = torch.zeros(n, dtype=torch.float32, device=dev)
        first = []
        for ms in mstate:
            first.append(ms is not None and bool(ms[0]) and not ms[1])      # the group's first step: its buffers are clones of the gradients
            for i in (ms[0] if ms is not None else ()):
                p, o = ps[i], offs[i]
                b = flat_b[o:o + p.numel()].view_as(p)
                if ms[1]:
                    b.copy_(self.state[p]["momentum_buffer"])
                self.state[p]["momentum_buffer"] = b
        return {"b": flat_b, "first": first, "mom_on": mom_on, "table": table, "seen": [None] * len(mstate)}

    def _flat_fits(self, f):
        # momentum switched on or off in a group after the layout was built: torch's path (it keeps or ignores the buffers by itself)
        return self._regroup or f["mom_on"] == [grp["momentum"] != 0 for grp in self.param_groups]

    def _launch(self, f, groups, gp, n):
        b, table, first, seen = f["b"], f["table"], f["first"], f["seen"]
        for g, grp in enumerate(groups):
            opts = (grp["lr"], grp["momentum"], grp["dampening"], grp["weight_decay"], grp["nesterov"], grp["maximize"], first[g])
            if opts != seen[g]:                           # (an entry is rewritten only when the group's options moved: a scheduler's lr)
                seen[g] = opts
                t = table[g]
                t.lr, t.momentum, t.dampening, t.weight_decay = float(opts[0]), float(opts[1]), float(opts[2]), float(opts[3])
                t.nesterov, t.maximize, t.first = int(bool(opts[4])), int(bool(opts[5])), int(opts[6])
        _lib.check(_lib.load().mlsp_sgd_flat_groups_f32(f["p"].data_ptr(), b.data_ptr() if b is not None else None, f["seg"][0], f["seg"][1], gp,
                                                        f["seg_group"], n, table, len(table), f["tile_amax"].data_ptr(), _lib.stream()),
                   "mlsp_sgd_flat_groups_f32")
        if any(first):
            f["first"] = [False] * len(first)
