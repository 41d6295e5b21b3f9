"""AdamW over LM_Net's flat parameter / gradient buffers: ONE kernel per step.

The reference trains with ``torch.optim.AdamW(model.parameters(), lr, weight_decay)`` (``train.py:156``) and a
``CosineAnnealingLR`` on top of it (``train.py:160``).  ``LM_Net`` already writes every gradient into one flat
fp32 buffer (``LM_Net._new_grads``); this optimizer lays the PARAMETERS out the same way (each ``p.data`` becomes a
view of one buffer, same offsets as its gradient) so that the whole update is a single ``lmn_adamw_step`` launch over
~4 M floats instead of ~90 multi-tensor launches over 514 tensors.

It is a ``torch.optim.Optimizer``, so LR schedulers, ``zero_grad`` and ``state_dict`` work as with the reference's
optimizer; ``state_dict()`` is emitted in ``torch.optim.AdamW``'s per-parameter layout and ``load_state_dict`` accepts it,
so optimizer checkpoints written by the reference load here and vice versa.

Two routes.  ``FusedAdamW(model, lr, ...)`` with one group and none of the arguments below is the route above: one launch, the
step count kept on the host.  Anything else -- several parameter groups, a frozen group, ``max_norm``, ``skip_nonfinite``,
``ema_decay``, or a ``torch.amp.GradScaler`` stepping this optimizer -- takes the EXTENDED route (include/optim/lmnet_optim.h): a
deterministic reduction over the flat gradient leaves a small control block on the device (non-finite count, gradient norm, clip
coefficient, step count, bias corrections) and a second step kernel reads it.  Nothing about a step is decided on the host:
``step()`` does no synchronisation and no allocation there, and can be captured in a graph.

  * Groups: a list of dicts with ``params`` and optionally ``lr``, ``weight_decay``, ``frozen``; they must partition
    ``model.parameters()``.  ``decay_groups(model, weight_decay)`` builds the usual decay / no-decay pair.  A frozen group is not
    read by the norm, not counted by the non-finite check and not stored by the step.  It saves NO backward time: LM_Net's single
    autograd node still forms every gradient.
  * Clipping: ``max_norm`` is ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` over the non-frozen groups, folded into the step.
    The gradient buffer is read-only: ``p.grad`` is NOT unscaled or clipped in place.  ``opt.grad_norm`` is the norm before clipping.
  * GradScaler: the reference's ``--apm`` lines ``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`` work unchanged.
    ``_step_supports_amp_scaling`` makes the scaler hang ``grad_scale`` and ``found_inf`` on the optimizer instead of unscaling 514
    tensors and reading ``found_inf`` back; ``step()`` passes their device pointers on.  Under a scaler a step with a non-finite
    gradient is always skipped: parameters, moments, EMA and ``device_step`` stay as they were, ``opt.skipped`` counts it.
  * EMA: ``ema_decay=d`` keeps ``opt.ema`` (flat, initialised to the parameters) as ``d * ema + (1 - d) * p`` after every step that is
    taken; ``with opt.swap_ema():`` evaluates with the averaged weights.  BatchNorm buffers (running statistics) are not averaged.
  * Data parallel: ``lm_net_amd.ddp.GradReducer.finish`` runs at the end of ``backward()`` and makes the compute stream wait for every
    collective, so the flat gradient is final -- averaged over the ranks -- for everything enqueued after ``backward()`` returns.
    ``step()`` enqueues on that stream: the norm is that of the averaged gradient, identical on every rank, and so is the decision
    to skip.
"""
import contextlib

import torch

from . import hip


class ParamGroups(list):
    """A list of parameter-group dicts that remembers the model it partitions (what ``decay_groups`` returns)."""
    model = None


def decay_groups(model, weight_decay=1e-2, no_decay=("bias",), lr=None):
    """The usual two groups: every parameter whose name ends in one of ``no_decay`` or that is 1-D (norm scales and shifts, biases)
    gets weight_decay 0, the rest ``weight_decay``.  Parameters with requires_grad=False go into a third, frozen group."""
    net = getattr(model, "module", model)
    decay, plain, frozen = [], [], []
    for name, p in net.named_parameters():
        if not p.requires_grad:
            frozen.append(p)
        elif p.dim() <= 1 or any(name.endswith(s) for s in no_decay):
            plain.append(p)
        else:
            decay.append(p)
    groups = ParamGroups()
    groups.model = net
    for params, extra in ((decay, dict(weight_decay=weight_decay)), (plain, dict(weight_decay=0.0)), (frozen, dict(frozen=True))):
        if params:
            g = dict(params=params, **extra)
            if lr is not None:
                g["lr"] = lr
            groups.append(g)
    return groups


def quad_groups(spans, gids, total):
    """uint8 [total / 4]: the group of every quad of the flat layout.  spans: (first, end) float offsets per parameter, every first a
    multiple of 4 (``LM_Net._ensure_grad_layout`` keeps each parameter 16-byte aligned, so no quad straddles two parameters); gids:
    the parameter's group.  The padding quad at a parameter's end belongs to that parameter's group; the spans must cover every
    quad exactly once."""
    if total % 4:
        raise ValueError("quad_groups: total=%d is not a multiple of 4" % total)
    q = torch.full((total // 4,), 255, dtype=torch.uint8)
    for (a, b), gid in zip(spans, gids):
        if a % 4 or not 0 <= a < b <= total:
            raise ValueError("quad_groups: span (%d, %d) is not 16-byte aligned inside [0, %d)" % (a, b, total))
        if not 0 <= gid < hip.OPTIM_MAX_GROUPS:
            raise ValueError("quad_groups: group %d outside [0, %d)" % (gid, hip.OPTIM_MAX_GROUPS))
        lo, hi = a // 4, (b + 3) // 4
        if bool((q[lo:hi] != 255).any()):
            raise ValueError("quad_groups: span (%d, %d) shares a quad with another parameter" % (a, b))
        q[lo:hi] = gid
    if bool((q == 255).any()):
        raise ValueError("quad_groups: %d quads belong to no parameter" % int((q == 255).sum()))
    return q


def _check_partition(all_params, groups):
    """groups (dicts) must partition all_params; a requires_grad=False parameter must sit in a frozen group."""
    seen = {}
    for gi, g in enumerate(groups):
        if not isinstance(g, dict) or "params" not in g:
            raise TypeError("FusedAdamW: a parameter group is a dict with a `params` list")
        for p in g["params"]:
            if id(p) in seen:
                raise ValueError("FusedAdamW: a parameter appears in groups %d and %d" % (seen[id(p)], gi))
            seen[id(p)] = gi
            if not p.requires_grad and not g.get("frozen", False):
                raise ValueError("FusedAdamW: a parameter with requires_grad=False is accepted only in a frozen group "
                                 "(dict(params=[...], frozen=True)); group %d is not frozen" % gi)
    ids = {id(p) for p in all_params}
    if set(seen) - ids:
        raise ValueError("FusedAdamW: %d grouped parameters do not belong to the model" % len(set(seen) - ids))
    if ids - set(seen):
        raise ValueError("FusedAdamW: the groups must partition model.parameters(): %d parameters are in no group" % len(ids - set(seen)))
    if not 1 <= len(groups) <= hip.OPTIM_MAX_GROUPS:
        raise ValueError("FusedAdamW: %d parameter groups (1..%d are supported)" % (len(groups), hip.OPTIM_MAX_GROUPS))
    return seen


def pack_state(param_groups, offs, exp_avg, exp_avg_sq, step):
    """The flat moments as a torch.optim.AdamW state dict: state[i] = {step, exp_avg, exp_avg_sq}, i counting through the groups'
    parameters in order; param_groups with indices for `params`.  offs: id(parameter) -> (first, end) in the flat buffers."""
    state, groups, i = {}, [], 0
    for grp in param_groups:
        out = {k: v for k, v in grp.items() if k != "params"}
        out["params"] = list(range(i, i + len(grp["params"])))
        groups.append(out)
        for p in grp["params"]:
            a, b = offs[id(p)]
            state[i] = dict(step=torch.tensor(float(step)),
                            exp_avg=exp_avg[a:b].view(p.shape).clone(),
                            exp_avg_sq=exp_avg_sq[a:b].view(p.shape).clone())
            i += 1
    return dict(state=state, param_groups=groups)


def unpack_state(sd, param_groups, offs, exp_avg, exp_avg_sq):
    """The inverse of pack_state, into the flat moments and the groups' hyper-parameters; -> the shared step count.  Accepts what
    torch.optim.AdamW writes, which keeps no state for a parameter that never had a gradient (a frozen one)."""
    if len(sd["param_groups"]) != len(param_groups):
        raise ValueError("FusedAdamW: the state dict has %d parameter groups, the optimizer %d"
                         % (len(sd["param_groups"]), len(param_groups)))
    params = []
    for grp, saved in zip(param_groups, sd["param_groups"]):
        if len(saved["params"]) != len(grp["params"]):
            raise ValueError("FusedAdamW: a parameter group of the state dict differs in size")
        for k, v in saved.items():
            if k != "params":
                grp[k] = v
        grp.setdefault("frozen", False)
        params += grp["params"]
    steps = set()
    for i, st in sd["state"].items():
        p = params[int(i)]
        a, b = offs[id(p)]
        exp_avg[a:b].copy_(st["exp_avg"].reshape(-1))
        exp_avg_sq[a:b].copy_(st["exp_avg_sq"].reshape(-1))
        steps.add(int(float(st["step"])))
    if len(steps) > 1:
        raise ValueError("FusedAdamW: per-parameter step counts differ; one shared count is kept")
    return steps.pop() if steps else 0


class FusedAdamW(torch.optim.Optimizer):
    _step_supports_amp_scaling = True      # GradScaler.step hangs grad_scale / found_inf on the optimizer and calls step() as is
    _SLOTS = 8                             # pinned staging rows of the group table

    def __init__(self, model_or_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, skip_nonfinite=False,
                 ema_decay=None, model=None):
        if isinstance(model_or_groups, torch.nn.Module):
            model, groups = model_or_groups, None
        else:
            groups = list(model_or_groups)
            model = model if model is not None else getattr(model_or_groups, "model", None)
            if model is None:
                raise TypeError("FusedAdamW: parameter groups need the model they partition: FusedAdamW(groups, ..., model=net) "
                                "(optim.decay_groups(net, ...) carries it)")
        net = getattr(model, "module", model)          # accept the DDP wrapper
        if not hasattr(net, "_ensure_grad_layout"):
            raise TypeError("FusedAdamW needs an lm_net_amd.LM_Net (flat gradient layout)")
        self.net = net
        params = list(net.parameters())
        if groups is None:
            if any(not p.requires_grad for p in params):
                raise ValueError("FusedAdamW(model): a parameter with requires_grad=False is accepted only in a frozen group: pass "
                                 "parameter groups with dict(params=[...], frozen=True) (optim.decay_groups builds them)")
            groups = [dict(params=params)]
        gid = _check_partition(params, groups)
        for g in groups:
            for k in ("betas", "eps"):
                if k in g and g[k] != dict(betas=betas, eps=eps)[k]:
                    raise ValueError("FusedAdamW: `%s` is shared by all groups" % k)
        if max_norm is not None and not max_norm > 0:
            raise ValueError("FusedAdamW: max_norm=%r must be positive (None: no clipping)" % (max_norm,))
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError("FusedAdamW: ema_decay=%r outside [0, 1]" % (ema_decay,))
        if not params or not params[0].is_cuda:
            raise RuntimeError("FusedAdamW: move the model to the GPU first (the HIP path has no CPU fallback)")
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, frozen=False))
        self.max_norm, self.skip_nonfinite, self.ema_decay = max_norm, bool(skip_nonfinite), ema_decay
        self._flatten_parameters()
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        self._host_step = 0
        L = self._layout
        self._frozen_ok = {id(p) for g in self.param_groups if g["frozen"] for p in g["params"]}
        live = [p for p in L["order"] if p.requires_grad] or L["order"]
        self._probes = (live[0], live[-1], live[len(live) // 2])
        # ---- the extended route's device state (a few KB and one byte per quad: always there, so that a GradScaler can switch to it)
        dev, n = self.flat_p.device, L["total"]
        self._qgroup = quad_groups([L["offs"][id(p)] for p in L["order"]], [gid[id(p)] for p in L["order"]], n).to(dev)
        self._ws = torch.zeros(hip.optim_workspace_words(n), device=dev, dtype=torch.float32)
        c0 = 2 * hip.optim_blocks(n)
        ctrl = self._ws[c0:c0 + hip.OPTIM_CTRL_WORDS]
        self._table = self._ws[c0 + hip.OPTIM_CTRL_WORDS:c0 + hip.OPTIM_CTRL_WORDS + hip.OPTIM_GROUP_WORDS]
        self.grad_norm = ctrl[hip.OPTIM_GRAD_NORM]                          # device views of the control block
        self.skipped = ctrl.view(torch.int32)[hip.OPTIM_SKIPPED]
        self.device_step = ctrl.view(torch.int32)[hip.OPTIM_STEP]
        self.clip_coef = ctrl[hip.OPTIM_COEF]
        self._stage = torch.zeros(self._SLOTS, hip.OPTIM_GROUP_WORDS, dtype=torch.float32).pin_memory()
        self._stage_ev = [None] * self._SLOTS
        self._slot = 0
        self._table_vals = None
        self.ema = self.flat_p.clone() if ema_decay is not None else None
        self.extended = (len(self.param_groups) > 1 or bool(self._frozen_ok) or max_norm is not None or self.skip_nonfinite
                         or ema_decay is not None)
        self._params_c = {}
        if self.extended:
            self.sync_groups()

    # ------------------------------------------------------------------ layout
    def _flatten_parameters(self):
        L = self.net._ensure_grad_layout()
        flat = torch.zeros(L["total"], device=L["device"], dtype=torch.float32)
        with torch.no_grad():
            for p in L["order"]:
                a, b = L["offs"][id(p)]
                flat[a:b].copy_(p.detach().reshape(-1))
                p.data = flat[a:b].view(p.shape)
        self.flat_p, self._layout = flat, L

    def _flat_grad(self):
        """The model's flat gradient buffer if every p.grad is still its view, else a gathered copy."""
        L, net = self._layout, self.net
        flat = getattr(net, "_grad_flat", None)
        ok = flat is not None and flat.numel() == L["total"] and all(p.requires_grad or id(p) in self._frozen_ok
                                                                     for p in L["order"][::37])
        if ok:
            for p in self._probes:
                a, _ = L["offs"][id(p)]
                if p.grad is None or p.grad.data_ptr() != flat.data_ptr() + 4 * a:
                    ok = False
                    break
        if ok:
            return flat
        g = torch.zeros_like(self.flat_p)
        for p in L["order"]:
            if p.grad is not None:
                a, b = L["offs"][id(p)]
                g[a:b].copy_(p.grad.reshape(-1))
        return g

    # ------------------------------------------------------------------ the extended route's host side
    @property
    def step_count(self):
        """Steps taken.  On the extended route the count lives on the device: reading it synchronises (state_dict does)."""
        return int(self.device_step.item()) if self.extended else self._host_step

    @step_count.setter
    def step_count(self, v):
        self._host_step = int(v)
        self.device_step.fill_(int(v))

    def _group_values(self):
        return [(float(g["lr"]), float(g["weight_decay"]), bool(g["frozen"])) for g in self.param_groups]

    def sync_groups(self):
        """Copy every group's lr / weight_decay / frozen to the device table (pinned staging row, non-blocking copy) if any of them
        changed.  ``step()`` does this by itself; inside a captured graph it cannot: call it after ``scheduler.step()``, outside
        the graph."""
        vals = self._group_values()
        if vals == self._table_vals:
            return False
        s = self._slot
        self._slot = (s + 1) % self._SLOTS
        if self._stage_ev[s] is not None and not self._stage_ev[s].query():
            self._stage_ev[s].synchronize()         # (the copy that last read this row, _SLOTS table changes ago: finished long since)
        row = self._stage[s]
        row.zero_()
        for k, (lr, wd, frozen) in enumerate(vals):
            row[4 * k], row[4 * k + 1], row[4 * k + 2] = lr, wd, 1.0 if frozen else 0.0
        self._table.copy_(row, non_blocking=True)
        if self._stage_ev[s] is None:
            self._stage_ev[s] = torch.cuda.Event()
        self._stage_ev[s].record()
        self._table_vals = vals
        return True

    def _param_c(self, scaled):
        """The OptimParam of this step (cached per flag set: built once)."""
        grp = self.param_groups[0]
        key = (bool(scaled), tuple(grp["betas"]), grp["eps"], self.max_norm, self.ema_decay, len(self.param_groups))
        p = self._params_c.get(key)
        if p is None:
            flags = hip.OPTIM_SKIP_NONFINITE if (self.skip_nonfinite or scaled) else 0
            p = self._params_c[key] = hip.optim_param(grp["betas"], grp["eps"], self.max_norm, self.ema_decay, flags, len(self.param_groups))
        return p

    # ------------------------------------------------------------------ Optimizer API
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = self._layout
        p0 = L["order"][0]
        if p0.data_ptr() != self.flat_p.data_ptr() + 4 * L["offs"][id(p0)][0]:
            raise RuntimeError("FusedAdamW: parameter storage was replaced after the optimizer was built "
                               "(model.to()/load via .data=); rebuild the optimizer")
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        scaled = grad_scale is not None or found_inf is not None
        if scaled and not self.extended:            # a GradScaler steps this optimizer: the device takes the count over, for good
            self.extended = True
            self.device_step.fill_(self._host_step)
        if not self.extended:
            grp = self.param_groups[0]
            b1, b2 = grp["betas"]
            self._host_step += 1
            hip.adamw_step(self.flat_p, self._flat_grad(), self.exp_avg, self.exp_avg_sq, grp["lr"], b1, b2, grp["eps"],
                           grp["weight_decay"], 1.0 - b1 ** self._host_step, 1.0 - b2 ** self._host_step)
            return loss
        if self._group_values() != self._table_vals:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: a group's lr / weight_decay changed inside a graph capture; call opt.sync_groups() "
                                   "after scheduler.step(), outside the graph")
            self.sync_groups()
        param, g = self._param_c(scaled), self._flat_grad()
        hip.optim_prepare(g, self._qgroup, param, self._ws, grad_scale, found_inf)
        hip.adamw_step_ex(self.flat_p, g, self.exp_avg, self.exp_avg_sq, self.ema, self._qgroup, param, self._ws)
        return loss

    @contextlib.contextmanager
    def swap_ema(self):
        """Evaluate with the averaged weights: parameter and EMA values are exchanged inside the block and exchanged back after it
        (bit for bit).  BatchNorm running statistics are not averaged: the model keeps those of the last training step."""
        if self.ema is None:
            raise RuntimeError("FusedAdamW.swap_ema: built without ema_decay")

        def swap():
            with torch.no_grad():
                tmp = self.flat_p.clone()
                self.flat_p.copy_(self.ema)
                self.ema.copy_(tmp)
        swap()
        try:
            yield self
        finally:
            swap()

    def state_dict(self):
        """torch.optim.AdamW layout: state[i] = {step, exp_avg, exp_avg_sq}, i counting through the groups' parameters in order."""
        return pack_state(self.param_groups, self._layout["offs"], self.exp_avg, self.exp_avg_sq, self.step_count)

    def load_state_dict(self, sd):
        self.step_count = unpack_state(sd, self.param_groups, self._layout["offs"], self.exp_avg, self.exp_avg_sq)
        if self.extended:
            self.sync_groups()
