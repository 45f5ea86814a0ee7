"""Adam / AdamW as one update launch over the whole parameter list, with the gradients' global norm, clipping by it and a guard against a
non-finite gradient formed on the device (csrc/optimizer.hip).

``FusedAdam`` is the product (HIP tensors only); ``FusedAdamTorch`` is the same class as plain torch ops on any device, every fp32
operation on its own and the scalars in Python floats -- the restatement the tests compare against bit for bit.  Nothing routes to it.

State (an fp64 tensor of 8 slots on the parameters' device): [0] t, completed steps; [1] beta1^t; [2] beta2^t (running products: one
IEEE multiplication per step, so a host restatement gets the same bits); [3] learning rate; [4] total gradient norm of the last step;
[5] the clip coefficient it used (an fp32 value); [6] skipped steps; [7] non-finite flag of the last step.  ``exp_avg`` and
``exp_avg_sq`` are two flat fp32 buffers, each tensor's segment starting at a multiple of four elements; the per-parameter state
tensors are views into them.

One step, for every tensor that has a gradient (a tensor whose ``.grad`` is None is left out and keeps p, m, v; the step count is
global, which differs from torch's per-tensor count for such tensors only):

    B1 = state[1] * beta1            B2 = state[2] * beta2                        (double)
    step_size = (float)(lr / (1 - B1))        sbc2 = (float)sqrt(1 - B2)
    c = (float)min(1.0, max_norm / (norm + 1e-6))                                 (torch's clip_grad_norm_; only with max_norm)
    g = grad * c
    g = g + wd * p                            (weight_decay != 0, not decoupled: Adam's L2 term)
    p = p - (float)(lr * wd) * p              (weight_decay != 0, decoupled: AdamW)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + ((1 - beta2) * g) * g
    p = p - step_size * (m / (sqrtf(v) / sbc2 + eps))

with beta1, 1 - beta1, beta2, 1 - beta2, eps, wd rounded once from double to fp32.  ``grad`` is never written.  With
``skip_nonfinite`` a step whose squared norm is inf or NaN writes nothing, leaves t and the powers alone and adds 1 to state[6].
"""
import math

import torch

_TORCH_KEYS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


def _f32(x):
    """x (a Python float) rounded once to fp32, as a Python float"""
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


def _beta_power(beta, t):
    """beta^t as the step's running product: t multiplications in double"""
    b = 1.0
    for _ in range(t):
        b = b * beta
    return b


def clip_coefficient(norm, max_norm):
    """(float)min(1.0, max_norm / (norm + 1e-6)) as a Python float; a NaN norm gives NaN, as torch's clip_grad_norm_ does"""
    q = max_norm / (norm + 1e-6)
    return _f32(q if (q < 1.0 or q != q) else 1.0)


class _FusedAdamBase(torch.optim.Optimizer):
    _label = "FusedAdam"                  # what the messages call the optimizer

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_norm=None, skip_nonfinite=False,
                 **torch_keys):
        unknown = set(torch_keys) - set(_TORCH_KEYS)
        if unknown:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(unknown)}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **{**_TORCH_KEYS, **torch_keys}, decoupled=bool(decoupled),
                        max_norm=max_norm, skip_nonfinite=bool(skip_nonfinite))
        super().__init__(params, defaults)
        self._check_groups(self.param_groups)
        ps = self.param_groups[0]["params"]
        self._check_params(ps)
        dev = ps[0].device if ps else torch.device("cpu")
        self._offsets, total = [], 0
        for p in ps:
            self._offsets.append(total)
            total += -(-p.numel() // 4) * 4                                # every segment starts at a multiple of four elements
        self._total = total
        self._exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        lr0 = float(self.param_groups[0]["lr"])
        self._state = torch.tensor([0.0, 1.0, 1.0, lr0, 0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=dev)
        self._lr_sent = lr0
        for p, o in zip(ps, self._offsets):
            n = p.numel()
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": self._exp_avg[o:o + n].view(p.shape),
                             "exp_avg_sq": self._exp_avg_sq[o:o + n].view(p.shape)}
        self._constructed = True

    def add_param_group(self, param_group):
        """Refused once constructed: the moment buffers are laid out for the one group the constructor got."""
        if getattr(self, "_constructed", False):
            raise ValueError(f"{self._label}: one parameter group only; its parameters are fixed at construction")
        super().add_param_group(param_group)

    def _the_group(self):
        self._check_groups(self.param_groups)
        return self.param_groups[0]

    # ---- what is refused
    @classmethod
    def _check_group_values(cls, g):
        if g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError(f"{cls._label}: amsgrad and maximize are not supported")
        b1, b2 = g["betas"]
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"{cls._label}: betas must lie in [0, 1) (got {g['betas']})")
        if not g["lr"] >= 0.0 or not g["eps"] >= 0.0 or not g["weight_decay"] >= 0.0:
            raise ValueError(f"{cls._label}: lr, eps and weight_decay must be >= 0")
        if g.get("max_norm") is not None and not g["max_norm"] >= 0.0:
            raise ValueError(f"{cls._label}: max_norm must be None or >= 0")

    @classmethod
    def _check_groups(cls, groups):
        if len(groups) != 1:
            raise ValueError(f"{cls._label}: one parameter group only (got {len(groups)})")
        cls._check_group_values(groups[0])

    def _check_params(self, ps):
        for i, p in enumerate(ps):
            if p.dtype != torch.float32:
                raise ValueError(f"{self._label}: parameter {i} is {p.dtype}; fp32 only")
            if not p.is_contiguous():
                raise ValueError(f"{self._label}: parameter {i} is not contiguous")
            if p.device != ps[0].device:
                raise ValueError(f"{self._label}: parameter {i} is on {p.device}, parameter 0 on {ps[0].device}; one device only")

    # ---- device views for logging without a host read
    @property
    def grad_norm(self):
        """total gradient norm of the last step (fp64; NaN when neither clipping nor the guard is on)"""
        return self._state[4]

    @property
    def clip_coef(self):
        """the clip coefficient the last step used (an fp32 value held in fp64)"""
        return self._state[5]

    @property
    def skipped_steps(self):
        return self._state[6]

    def _needs_norm(self, g):
        return g["max_norm"] is not None or g["skip_nonfinite"]

    def push_lr(self):
        """Send ``param_groups[0]["lr"]`` to the device if it differs from the value last sent: one asynchronous write of state[3] on the
        current stream.  ``step()`` does this itself; call it between replays of a ``CapturedStep``, where ``step()`` does not run again."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_sent:
            if self._state.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._label}: the learning rate changed inside a graph capture; call push_lr() before capturing")
            self._state[3:4].fill_(lr)
            self._lr_sent = lr

    # ---- checkpoints in torch.optim.Adam's format
    def state_dict(self):
        """As ``torch.optim.Adam.state_dict()``: state[i] = {"step" (fp32 CPU scalar), "exp_avg", "exp_avg_sq"} and one param group with
        torch's keys plus ``decoupled`` (also under torch's name ``decoupled_weight_decay``), ``max_norm``, ``skip_nonfinite`` and the
        counter ``skipped_steps``.  Reads the step count and the counter from the device (one host read)."""
        t, skipped = self._state[0].item(), self._state[6].item()
        for st in self.state.values():
            st["step"] = torch.tensor(t, dtype=torch.float32)
        sd = super().state_dict()
        for g in sd["param_groups"]:
            g["decoupled_weight_decay"] = g["decoupled"]
            g["skipped_steps"] = int(skipped)
        return sd

    def load_state_dict(self, state_dict):
        """Takes a dict saved by this class, by ``torch.optim.Adam`` or by ``torch.optim.AdamW``.  The moments are copied into the flat
        buffers (the per-parameter tensors stay views) and beta^t is rebuilt by t multiplications in double, so a resumed run continues
        bit for bit.  Per-tensor step counts that differ, more than one group, amsgrad or maximize raise ValueError.  Registered
        load_state_dict pre- and post-hooks run as they do for any optimizer; ``skipped_steps`` continues from the saved count (0 for a
        dict of torch's)."""
        for pre_hook in self._optimizer_load_state_dict_pre_hooks.values():
            hooked = pre_hook(self, state_dict)
            if hooked is not None:
                state_dict = hooked
        groups = state_dict["param_groups"]
        self._check_groups(groups)
        g = dict(groups[0])
        ids = list(g.pop("params"))
        ps = self.param_groups[0]["params"]
        if len(ids) != len(ps):
            raise ValueError(f"{self._label}: the loaded group has {len(ids)} parameters, this optimizer {len(ps)}")
        if "decoupled" not in g:
            g["decoupled"] = bool(g.get("decoupled_weight_decay", self.param_groups[0]["decoupled"]))
        g.pop("decoupled_weight_decay", None)
        g.pop("param_names", None)
        skipped = float(g.pop("skipped_steps", 0))
        g["betas"] = tuple(g["betas"])
        merged = {**self.param_groups[0], **g, "params": ps}
        self._check_group_values(merged)
        saved = state_dict["state"]
        steps = {float(st["step"]) for st in saved.values()}
        if len(steps) > 1:
            raise ValueError(f"{self._label}: per-tensor step counts differ ({sorted(steps)}); the step count here is global")
        t = steps.pop() if steps else 0.0
        if t != int(t) or t < 0:
            raise ValueError(f"{self._label}: step count {t}")
        for i, p in zip(ids, ps):
            st = saved.get(i)
            for key in ("exp_avg", "exp_avg_sq"):
                if st is not None and tuple(st[key].shape) != tuple(p.shape):
                    raise ValueError(f"{self._label}: {key} of parameter {i} has shape {tuple(st[key].shape)}, the parameter {tuple(p.shape)}")
        self.param_groups[0].update(merged)
        with torch.no_grad():
            for i, p in zip(ids, ps):
                st = saved.get(i)
                for key in ("exp_avg", "exp_avg_sq"):
                    if st is None:
                        self.state[p][key].zero_()
                    else:
                        self.state[p][key].copy_(st[key])
            b1, b2 = merged["betas"]
            lr = float(merged["lr"])
            head = torch.tensor([t, _beta_power(b1, int(t)), _beta_power(b2, int(t)), lr, 0.0, 1.0, skipped, 0.0], dtype=torch.float64)
            self._state.copy_(head)
            self._lr_sent = lr
        for post_hook in self._optimizer_load_state_dict_post_hooks.values():
            post_hook(self)


class FusedAdamTorch(_FusedAdamBase):
    """The arithmetic of ``FusedAdam`` as plain torch ops on any device (see the module docstring): each fp32 operation one by one, no
    addcmul or lerp, the scalars in Python floats, the norm in fp64."""

    @torch.no_grad()
    def step(self, closure=None, clip_coef=None):
        """``clip_coef``: the coefficient to use instead of the one formed from this side's own norm (the norm's last bits depend on the
        summation order; the tests hand over the device's)."""
        if closure is not None:
            raise ValueError("FusedAdam takes no closure")
        g = self._the_group()
        self.push_lr()
        lr, (beta1, beta2), eps, wd = float(g["lr"]), g["betas"], float(g["eps"]), float(g["weight_decay"])
        ps = [p for p in g["params"] if p.grad is not None and p.numel() > 0]
        if not ps:
            return
        t, b1p, b2p = self._state[:3].tolist()
        use_norm = self._needs_norm(g)
        c = None
        if clip_coef is not None:
            clip_coef = float(clip_coef)
            if clip_coef != _f32(clip_coef) and clip_coef == clip_coef:
                raise ValueError("clip_coef must be an fp32 value")
        if use_norm:
            total = sum(float((p.grad.double() * p.grad.double()).sum()) for p in ps)
            norm = math.sqrt(total) if total == total else total
            flag = not (total < math.inf)
            c = clip_coefficient(norm, float(g["max_norm"])) if g["max_norm"] is not None else 1.0
            c = clip_coef if clip_coef is not None else c                      # state[5]: the coefficient this step uses
            self._state[4], self._state[5], self._state[7] = norm, c, float(flag)
            if g["skip_nonfinite"] and flag:
                self._state[6] += 1.0
                return
        else:
            c = clip_coef
            self._state[4], self._state[5], self._state[7] = math.nan, 1.0 if c is None else c, 0.0
        B1, B2 = b1p * beta1, b2p * beta2
        step_size, sbc2 = _f32(lr / (1.0 - B1)), _f32(math.sqrt(1.0 - B2))
        b1f, omb1f, b2f, omb2f = _f32(beta1), _f32(1.0 - beta1), _f32(beta2), _f32(1.0 - beta2)
        epsf, wdf, lrwdf = _f32(eps), _f32(wd), _f32(lr * wd)
        for p in ps:
            st = self.state[p]
            m, v = st["exp_avg"], st["exp_avg_sq"]
            grad = p.grad * c if c is not None else p.grad
            if wd != 0.0 and not g["decoupled"]:
                grad = grad + p * wdf
            if wd != 0.0 and g["decoupled"]:
                p.copy_(p - p * lrwdf)
            m.copy_(m * b1f + grad * omb1f)
            v.copy_(v * b2f + (grad * omb2f) * grad)
            # (sqrtf correctly rounded on every device: through fp64, whose 53 >= 2 * 24 + 2 bits make the second rounding harmless.
            #  torch's own fp32 sqrt carries no such guarantee: tests/test_fused_optimizer.py names an input where a CPU build differs)
            p.copy_(p - (m / (v.double().sqrt().to(torch.float32) / sbc2 + epsf)) * step_size)
        self._state[0], self._state[1], self._state[2] = t + 1.0, B1, B2


class FusedAdam(_FusedAdamBase):
    """``FusedAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_norm=None, skip_nonfinite=False)``:
    Adam (``decoupled=False``: weight decay as an L2 term) or AdamW (``decoupled=True``) over fp32 HIP parameters of one group, the whole
    list in one update launch and one closing wave; with ``max_norm`` the gradients are scaled as ``torch.nn.utils.clip_grad_norm_`` would
    scale them (two more launches, ``grad`` itself untouched); with ``skip_nonfinite`` a step with an inf or NaN gradient changes nothing
    and is counted in ``skipped_steps``.  ``zero_grad``, ``param_groups`` and ``torch.optim.lr_scheduler.*`` work as for any optimizer.
    Capturable as it stands (no host read in ``step()``); inside a ``CapturedStep`` a new learning rate is sent with ``push_lr()``."""

    def _check_params(self, ps):
        from ._lib import SminHipError
        for i, p in enumerate(ps):
            if not p.is_cuda:
                raise SminHipError(f"FusedAdam runs on a HIP device only (parameter {i} is a CPU tensor); there is no CPU fallback -- the "
                                   "plain-torch restatement is available under the explicit name FusedAdamTorch")
        super()._check_params(ps)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_norm=None, skip_nonfinite=False,
                 **torch_keys):
        super().__init__(params, lr, betas, eps, weight_decay, decoupled, max_norm, skip_nonfinite, **torch_keys)
        self._ws = None                                                    # the norm's partials; None until clipping or the guard is on

    def _workspace(self):
        if self._ws is None:
            from . import _lib
            ps = self.param_groups[0]["params"]
            nbytes = _lib.load().smin_adam_ws_bytes(sum(p.numel() for p in ps), len(ps))
            self._ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self._state.device)
        return self._ws

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdam takes no closure")
        from . import _lib
        g = self._the_group()
        self.push_lr()
        params, grads, offsets = [], [], []
        for p, o in zip(g["params"], self._offsets):
            if p.grad is not None:
                params.append(p)
                grads.append(p.grad)
                offsets.append(o)
        ws = self._workspace() if self._needs_norm(g) else None
        beta1, beta2 = g["betas"]
        _lib.load_torch().adam_step(params, grads, self._exp_avg, self._exp_avg_sq, offsets, self._state, ws, float(beta1), float(beta2),
                                    float(g["eps"]), float(g["weight_decay"]), bool(g["decoupled"]),
                                    float(g["max_norm"]) if g["max_norm"] is not None else -1.0, bool(g["skip_nonfinite"]))


# ---------------------------------------------------------------- lazy Adam over the rows of a word table
class _RowSparseAdamBase(_FusedAdamBase):
    """Adam over one ``(V, E)`` table whose gradient arrives as a ``sampling.RowSparseGrad``: only the rows a batch touched are read or
    written (lazy Adam, the rule of ``torch.optim.SparseAdam``: an untouched row keeps p, m and v), with ``FusedAdam``'s state, arithmetic
    and checkpoint format (``torch.optim.Adam``'s: ``step``, dense ``exp_avg`` / ``exp_avg_sq``).  t and the powers of the betas are global
    and advance once per consumed gradient.  No weight decay (it would move every row), amsgrad or maximize."""

    def __init__(self, table, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, skip_nonfinite=False, **torch_keys):
        if not isinstance(table, torch.Tensor):
            raise TypeError(f"{type(self).__name__}: exactly one table, a tensor (got {type(table).__name__})")
        wd = torch_keys.pop("weight_decay", 0.0)
        if wd != 0.0:
            raise ValueError(f"{type(self).__name__}: weight_decay is not supported (it would touch every row of the table)")
        super().__init__([table], lr, betas, eps, 0.0, False, None, skip_nonfinite, **torch_keys)

    _label = "RowSparseAdam"

    @classmethod
    def _check_group_values(cls, g):
        if g.get("weight_decay", 0.0) != 0.0 or g.get("max_norm") is not None:
            raise ValueError("RowSparseAdam: weight_decay and max_norm are not supported (pass the model's coefficient as step(scale=...))")
        super()._check_group_values(g)

    def _check_params(self, ps):
        super()._check_params(ps)
        if ps[0].dim() != 2 or ps[0].shape[0] < 1 or ps[0].shape[1] < 4 or ps[0].shape[1] % 4:
            raise ValueError(f"RowSparseAdam: the table must be (V >= 1, E) with E % 4 == 0 (got {tuple(ps[0].shape)})")

    @property
    def table(self):
        return self.param_groups[0]["params"][0]

    def _pending(self):
        rg = getattr(self.table, "row_grad", None)
        return rg if rg is not None and rg.pending else None

    def zero_grad(self, set_to_none=True):
        rg = getattr(self.table, "row_grad", None)
        if rg is not None:
            rg.clear()
            if set_to_none:
                self.table.row_grad = None
        super().zero_grad(set_to_none)


def _scale_f32(scale):
    """the scale as the update uses it: cast once to fp32 (a Python float; reads a device value)"""
    x = scale.detach().reshape(-1)[0].item() if isinstance(scale, torch.Tensor) else float(scale)
    return _f32(x)


class RowSparseAdamTorch(_RowSparseAdamBase):
    """The arithmetic of ``RowSparseAdam`` as plain torch ops on any device, written as ``FusedAdamTorch`` is: each fp32 operation one by
    one, the scalars in Python floats.  ``step(grad)`` takes a ``RowSparseGrad`` or a pair ``(ids, rows)`` of distinct row indices (an id
    outside ``[0, V)`` is ignored, as the -1 of an unused slot) and their gradient rows.  Nothing routes to it."""

    @torch.no_grad()
    def step(self, grad=None, scale=None, closure=None):
        if closure is not None:
            raise ValueError("RowSparseAdam takes no closure")
        g = self._the_group()
        self.push_lr()
        if grad is None:
            grad = self._pending()
            if grad is None:
                return
        p, V = self.table, self.table.shape[0]
        if isinstance(grad, (tuple, list)):
            ids, rows = grad
            ids = torch.as_tensor(ids, device=p.device).to(torch.int64)
            rows = torch.as_tensor(rows, device=p.device).to(torch.float32).reshape(ids.shape[0], -1)
            keep = (ids >= 0) & (ids < V)
            ids, rows = ids[keep], rows[keep]
            total = float((rows.double() * rows.double()).sum())
        else:
            ids = grad.ids.to(device=p.device, dtype=torch.int64)
            keep = (ids >= 0) & (ids < V)
            ids, rows = ids[keep], grad.rows.to(p.device)[keep]
            total = float(grad.sq_norm.reshape(-1)[0])
            grad.clear()
        lr, (beta1, beta2), eps = float(g["lr"]), g["betas"], float(g["eps"])
        t, b1p, b2p = self._state[:3].tolist()
        c = None if scale is None else _scale_f32(scale)
        flag = not (total < math.inf) or (c is not None and not (abs(c) < math.inf))
        self._state[4], self._state[5], self._state[7] = (math.sqrt(total) if total >= 0.0 else math.nan), 1.0 if c is None else c, float(flag)
        if g["skip_nonfinite"] and flag:
            self._state[6] += 1.0
            return
        B1, B2 = b1p * beta1, b2p * beta2
        step_size, sbc2 = _f32(lr / (1.0 - B1)), _f32(math.sqrt(1.0 - B2))
        b1f, omb1f, b2f, omb2f, epsf = _f32(beta1), _f32(1.0 - beta1), _f32(beta2), _f32(1.0 - beta2), _f32(eps)
        st = self.state[p]
        m, v = st["exp_avg"], st["exp_avg_sq"]
        gr = rows * c if c is not None else rows
        m_r = m[ids] * b1f + gr * omb1f
        v_r = v[ids] * b2f + (gr * omb2f) * gr
        p_r = p[ids] - (m_r / (v_r.double().sqrt().to(torch.float32) / sbc2 + epsf)) * step_size
        m[ids], v[ids], p[ids] = m_r, v_r, p_r
        self._state[0], self._state[1], self._state[2] = t + 1.0, B1, B2


class RowSparseAdam(_RowSparseAdamBase):
    """``RowSparseAdam(table, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, skip_nonfinite=False)``: lazy Adam over one fp32, contiguous HIP
    ``(V, E)`` table trained through ``embed_tokens(..., differentiable=True, sparse_grad=True)``.  ``step(scale=None)`` consumes
    ``table.row_grad`` in two launches sized by the batch (``smin_row_adam_step``): the rows listed there get ``FusedAdam``'s update, every
    other row of the table and of the moments is neither read nor written; without a pending gradient it does nothing and t stays.
    ``scale``: a device fp64 value (or a float) the gradient rows are multiplied by, e.g. ``FusedAdam.clip_coef`` of the model's optimizer
    after its step.  With ``skip_nonfinite`` a gradient whose ``sq_norm``, or a ``scale`` that, is inf or NaN changes nothing and is
    counted in ``skipped_steps``.  ``grad_norm`` is the row gradient's own norm.  No host read; ``push_lr``, ``zero_grad``,
    ``state_dict`` / ``load_state_dict`` and ``torch.optim.lr_scheduler.*`` as for ``FusedAdam``."""

    def _check_params(self, ps):
        from ._lib import SminHipError
        if not ps[0].is_cuda:
            raise SminHipError("RowSparseAdam runs on a HIP device only (the table is a CPU tensor); there is no CPU fallback -- the "
                               "plain-torch restatement is available under the explicit name RowSparseAdamTorch")
        super()._check_params(ps)
        if ps[0].data_ptr() % 16:
            raise ValueError("RowSparseAdam: the table must be 16-byte aligned")

    @torch.no_grad()
    def step(self, scale=None, closure=None):
        if closure is not None:
            raise ValueError("RowSparseAdam takes no closure")
        from ._lib import call, ptr, stream
        g = self._the_group()
        self.push_lr()
        rg = self._pending()
        if rg is None:
            return
        p = self.table
        V, E = p.shape
        if rg.shape != (V, E) or rg.rows.device != p.device:
            raise ValueError(f"RowSparseAdam: row_grad is of a {rg.shape} table on {rg.rows.device}, the table {(V, E)} on {p.device}")
        if scale is not None:
            if not isinstance(scale, torch.Tensor):
                scale = torch.full((1,), float(scale), dtype=torch.float64).to(p.device, non_blocking=True)
            if scale.dtype != torch.float64 or scale.numel() != 1 or scale.device != p.device:
                raise ValueError("RowSparseAdam: scale must be one fp64 value on the table's device (or a float)")
            scale = scale.detach().contiguous()
        beta1, beta2 = g["betas"]
        with torch.cuda.device(p.device):
            call("smin_row_adam_step", stream(), ptr(p.detach()), ptr(self._exp_avg), ptr(self._exp_avg_sq), ptr(rg.ids), ptr(rg.rows),
                 ptr(rg.count), ptr(rg.sq_norm), rg.ids.shape[0], V, E, ptr(self._state), ptr(scale), float(beta1), float(beta2),
                 float(g["eps"]), int(bool(g["skip_nonfinite"])))
        rg.clear()
