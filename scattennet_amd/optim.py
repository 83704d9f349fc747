"""The training update on the HIP path: gradient clipping + Adam in two launches.

The reference's step (opt.py:28-38) ends with `clip_grad_norm_(model.parameters(), 1.0)` and
`optimizer.step()` of the `torch.optim.Adam` built by optimizer.py:33-66 (one parameter group
per model child; "adamw" is plain Adam there too), skipped when the loss is not finite.
`FusedAdam` does all of that in `sca_optim_grad_sqnorm` + `sca_optim_adam_step`
(csrc/optim.hip) over every parameter tensor at once, without a host sync, so the update can
sit in the same hipGraph as the forward and the backward.

The kernels are driven by tables in device memory:

* tensor table — per parameter with a gradient: pointers to p, g, exp_avg, exp_avg_sq and (amsgrad)
  max_exp_avg_sq, element count, group index and `t0` (the optimizer's step count before the
  tensor's first update: torch keeps one step count per parameter);
* chunk table — (tensor, offset, length) pieces of `CHUNK` elements (`plan_chunks`);
* group table — lr, betas, eps, weight decay of every parameter group, as doubles;
* state block — step, skipped, grad_norm, clip_coef (`opt.grad_norm`, `opt.clip_coef`,
  `opt.skipped`, `opt.step_count` are device views of it).

Table upkeep.  An eager `step()` compares every `p.grad.data_ptr()` with the table it last
uploaded and rebuilds only on change.  Under stream capture the step always uploads a table
of its own, taken from a small pool allocated beforehand (`capture_slots`, by default
`SPARE_TABLES`; one per captured step, e.g. one per length bucket), with an
asynchronous copy from a pinned host buffer that is never written again and lives as long
as the optimizer: replaying the copy node is harmless, and no eager step ever touches a
table a graph reads.  The group table is not part of that upload: `sync_hyperparameters()`
refreshes it between replays (an eager `step()` calls it when a value changed).

Capture protocol: one eager `step()` first (it allocates moments, tables and workspace),
then capture forward + backward + `step()`; call `sync_hyperparameters()` outside the graph
after a scheduler step.

`t0` is counted on the host (`step()` calls since construction or `load_state_dict`): a
tensor whose FIRST gradient arrives after skipped steps or graph replays gets its bias
correction from that count (`state_dict()` re-reads the device count).
"""
import ctypes
import math

import numpy as np
import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import _LRScheduler

from . import _lib

CHUNK = 8192        # elements per chunk (tools/optim_bench.py --chunk measures others)
SPARE_TABLES = 2    # tables a stream capture can take (one per captured step()): the default capture_slots
_ALIGN = 64         # floats: every moment slot starts on a 256-byte boundary

_TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"),
                       ("max_exp_avg_sq", "<u8"), ("numel", "<i8"), ("group", "<i4"), ("t0", "<i4")])
_CHUNK_DT = np.dtype([("tensor", "<i4"), ("len", "<i4"), ("offset", "<i8")])
_GROUP_DT = np.dtype([("lr", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("weight_decay", "<f8")])
assert _TENSOR_DT.itemsize == ctypes.sizeof(_lib.OptimTensor)
assert _CHUNK_DT.itemsize == ctypes.sizeof(_lib.OptimChunk)
assert _GROUP_DT.itemsize == ctypes.sizeof(_lib.OptimGroup)

_NO_CPU = ("scattennet_amd.optim runs only on ROCm (MI355X) fp32 tensors; got {} {}.  "
           "There is no CPU fallback.")


def plan_chunks(numels, chunk=CHUNK):
    """The chunk table for tensors of `numels` elements: a structured array (tensor, len,
    offset) that covers every element of every tensor exactly once, in tensor order, each
    chunk inside one tensor and at most `chunk` long (an empty tensor gets no chunk)."""
    numels = np.asarray(list(numels), dtype=np.int64).reshape(-1)
    if chunk < 1 or (numels < 0).any():
        raise ValueError("plan_chunks: chunk must be positive and sizes non-negative")
    counts = (numels + chunk - 1) // chunk
    total = int(counts.sum())
    out = np.zeros(total, dtype=_CHUNK_DT)
    tensor = np.repeat(np.arange(len(numels), dtype=np.int64), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)
    offset = (np.arange(total, dtype=np.int64) - first) * chunk
    out["tensor"] = tensor
    out["offset"] = offset
    out["len"] = np.minimum(chunk, numels[tensor] - offset)
    return out


def _chunk_count(numels, chunk):
    return sum((n + chunk - 1) // chunk for n in numels)


class _Retired:
    """Pinned host buffers of eager uploads, kept until the copy that reads them is done."""

    def __init__(self):
        self.items = []

    def add(self, host):
        ev = torch.cuda.Event()
        ev.record()
        self.items = [(e, h) for e, h in self.items if not e.query()]
        self.items.append((ev, host))


_RETIRED = _Retired()


def _upload(dev, host, nbytes):
    _lib.check(_lib.lib().sca_optim_upload(dev.data_ptr(), host.data_ptr(), nbytes, _lib.stream_handle()),
               "sca_optim_upload")


class _Tables:
    """One tensor table + chunk table: a device buffer and the pinned host image it is
    uploaded from."""

    def __init__(self, ntensors, nchunks, device, pinned=True):
        self.chunk_off = -(-max(ntensors, 1) * _TENSOR_DT.itemsize // 16) * 16
        self.nbytes = self.chunk_off + max(nchunks, 1) * _CHUNK_DT.itemsize
        self.cap = (ntensors, nchunks)
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.host = torch.empty(self.nbytes, dtype=torch.uint8).pin_memory() if pinned else None
        self.ntensors = self.nchunks = 0

    def upload(self, tensors, chunks, host=None):
        """Write the tables into the host image (`host`: a fresh pinned buffer for an eager
        upload) and enqueue the copy on the current stream."""
        assert len(tensors) <= self.cap[0] and len(chunks) <= self.cap[1]
        host = self.host if host is None else host
        img = host.numpy()
        img[:tensors.nbytes] = tensors.view(np.uint8)
        img[self.chunk_off:self.chunk_off + chunks.nbytes] = chunks.view(np.uint8)
        self.ntensors, self.nchunks = len(tensors), len(chunks)
        _upload(self.dev, host, self.nbytes)

    @property
    def tensors_ptr(self):
        return self.dev.data_ptr()

    @property
    def chunks_ptr(self):
        return self.dev.data_ptr() + self.chunk_off


def _check_tensor(t, what):
    if t.is_sparse:
        raise ValueError(f"{what}: sparse tensors are not supported")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: only fp32 is supported, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")


def _adam_group_keys():
    """torch.optim.Adam's param_group keys (same keys: checkpoints load either way)."""
    import inspect
    d = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
             capturable=False, differentiable=False, fused=None)
    if "decoupled_weight_decay" in inspect.signature(torch.optim.Adam.__init__).parameters:
        d["decoupled_weight_decay"] = False
    return d


_UNSUPPORTED = ("maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay")


class FusedAdam(Optimizer):
    """torch.optim.Adam (L2 weight decay, optional amsgrad) with clip_grad_norm_ folded in
    (`max_grad_norm`, None: no clipping) and the non-finite-loss skip of opt.py:32-37 on the
    device (`step(loss=...)`).  See the module docstring for the capture protocol;
    `capture_slots` is the number of captured `step()` calls the optimizer can take part in
    (one per graph, e.g. one per length bucket of `BucketedTrainStep`)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 max_grad_norm=None, *, max_blocks=0, chunk=CHUNK, capture_slots=SPARE_TABLES):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr must be a float (a tensor lr is torch's capturable path)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if max_blocks < 0 or chunk < 1:
            raise ValueError("FusedAdam: max_blocks must be >= 0 and chunk >= 1")
        if int(capture_slots) != capture_slots or capture_slots < 0:
            raise ValueError(f"FusedAdam: capture_slots must be a non-negative integer, got {capture_slots!r}")
        self.capture_slots = int(capture_slots)  # captured step() calls this optimizer can take part in
        self.max_grad_norm = max_grad_norm
        self.max_blocks = int(max_blocks)
        self.chunk = int(chunk)
        self._flat = []          # per group: {"exp_avg", "exp_avg_sq", "max_exp_avg_sq"} flat buffers
        self._slot = {}          # param -> (group index, offset, numel) in the group's flat buffers
        self._t0 = {}            # param -> optimizer step count before its first update
        self._calls = 0          # updates enqueued (host count)
        self._block = None       # device state block (int32 x 4)
        self._partials = None
        self._groups_dev = None
        self._hyper = None       # group-table values last uploaded
        self._eager = None       # the eager steps' table
        self._key = None         # what the eager table was built from
        self._spare, self._frozen = [], []
        self._capacity = None
        defaults = _adam_group_keys()
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------ construction
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            for k in _UNSUPPORTED:
                if group.get(k):
                    raise TypeError(f"FusedAdam does not support {k}={group[k]!r}")
            for p in group["params"]:
                _check_tensor(p, "FusedAdam parameter")
        except Exception:
            self.param_groups.pop()
            raise

    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                if not p.is_cuda:
                    raise RuntimeError(_NO_CPU.format(p.device, p.dtype))
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        raise ValueError("FusedAdam: no parameters")

    def _ensure_device(self, capturing=False):
        """Moments, state block, workspace and tables: allocated on the first eager step (and
        again when a parameter group was added).  Their sizes depend on the parameters only."""
        numels = [p.numel() for g in self.param_groups for p in g["params"]]
        capacity = (len(numels), _chunk_count(numels, self.chunk), len(self.param_groups),
                    tuple(bool(g["amsgrad"]) for g in self.param_groups))
        if capacity == self._capacity:
            return
        if capturing:
            raise RuntimeError("FusedAdam: run one eager step() before capturing (moments and tables are "
                               "allocated there, not while a stream is capturing)")
        dev = self._device()
        _lib.lib()
        if self._block is None:
            self._block = torch.zeros(4, dtype=torch.int32, device=dev)
            self._block.view(torch.float32)[3] = 1.0
            self._partials = torch.zeros(_lib.lib().sca_optim_blocks(self.max_blocks, 2 ** 31 - 1),
                                         dtype=torch.float32, device=dev)
        for gi, group in enumerate(self.param_groups):
            if gi == len(self._flat):
                off = 0
                for p in group["params"]:
                    self._slot[p] = (gi, off, p.numel())
                    off += -(-p.numel() // _ALIGN) * _ALIGN
                self._flat.append({k: torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
                                   for k in ("exp_avg", "exp_avg_sq")})
            if group["amsgrad"] and "max_exp_avg_sq" not in self._flat[gi]:
                self._flat[gi]["max_exp_avg_sq"] = torch.zeros_like(self._flat[gi]["exp_avg"])
        if self._groups_dev is not None:
            self._frozen.append(self._groups_dev)  # a captured graph may still read it
        self._groups_dev = torch.zeros(capacity[2] * _GROUP_DT.itemsize, dtype=torch.uint8, device=dev)
        self._hyper = None
        self._eager = _Tables(capacity[0], capacity[1], dev, pinned=False)
        self._key = None
        self._spare = [_Tables(capacity[0], capacity[1], dev) for _ in range(self.capture_slots)]
        self._capacity = capacity

    def _moment(self, p, name):
        gi, off, n = self._slot[p]
        return self._flat[gi][name][off:off + n].view(p.shape)

    # ------------------------------------------------------------------ tables
    def _scan(self):
        entries, key = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    entries.append((p, gi))
                    key.append((p.data_ptr(), g.data_ptr()))
        return entries, key

    def _build(self, entries):
        tensors = np.zeros(len(entries), dtype=_TENSOR_DT)
        for i, (p, gi) in enumerate(entries):
            g = p.grad
            _check_tensor(g, "FusedAdam gradient")
            if not g.is_cuda or g.device != p.device or g.shape != p.shape:
                raise ValueError(f"FusedAdam gradient: {tuple(g.shape)} on {g.device} for a parameter "
                                 f"{tuple(p.shape)} on {p.device}")
            st = self.state[p]
            if "exp_avg" not in st:  # first gradient: the state torch.optim.Adam would create
                self._t0[p] = self._calls
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = self._moment(p, "exp_avg")
                st["exp_avg_sq"] = self._moment(p, "exp_avg_sq")
            if self.param_groups[gi]["amsgrad"] and "max_exp_avg_sq" not in st:
                st["max_exp_avg_sq"] = self._moment(p, "max_exp_avg_sq")
            tensors[i] = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                          st["max_exp_avg_sq"].data_ptr() if self.param_groups[gi]["amsgrad"] else 0,
                          p.numel(), gi, self._t0[p])
        return tensors, plan_chunks([p.numel() for p, _ in entries], self.chunk)

    def _hyper_values(self):
        return [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                 float(g["weight_decay"])) for g in self.param_groups]

    def hyperparameters_changed(self):
        """True when lr, betas, eps or weight decay of a param_group differ from the device
        group table (a scheduler stepped): a replay needs `sync_hyperparameters()` first."""
        return self._hyper != self._hyper_values()

    def sync_hyperparameters(self):
        """Copy lr, betas, eps and weight decay of every param_group to the device group table
        (on the current stream).  Call it outside a captured graph, between replays, after a
        scheduler step; eager steps call it themselves when a value changed."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdam.sync_hyperparameters() must run outside stream capture")
        self._ensure_device()
        values = self._hyper_values()
        host = torch.empty(self._groups_dev.numel(), dtype=torch.uint8).pin_memory()
        host.numpy()[:] = np.array(values, dtype=np.float64).reshape(-1).view(np.uint8)
        _upload(self._groups_dev, host, host.numel())
        _RETIRED.add(host)
        self._hyper = values

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None, loss=None):
        """One clipped Adam update of every parameter that has a gradient: two launches on
        the current stream, no host sync.  `loss`: optional 0-d device tensor; when it is not
        finite the call changes nothing but `skipped` (parameters, moments and step count stay
        as they are)."""
        out = None
        if closure is not None:
            with torch.enable_grad():
                out = closure()
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        self._ensure_device(capturing)
        if loss is not None:
            loss = loss.detach()
            if not loss.is_cuda or loss.dtype != torch.float32 or loss.numel() != 1:
                raise ValueError("FusedAdam.step: loss must be a 0-d fp32 device tensor")
        entries, key = self._scan()
        if capturing:
            if self._hyper != self._hyper_values():
                raise RuntimeError("FusedAdam: hyper-parameters changed since the last eager step; call "
                                   "sync_hyperparameters() before capturing")
            if not self._spare:
                raise RuntimeError(f"FusedAdam: no spare table left for this capture ({self.capture_slots} captured "
                                   "steps per optimizer: scattennet_amd.optim.SPARE_TABLES); construct it with "
                                   "a larger capture_slots")
            tab = self._spare.pop()
            self._frozen.append(tab)  # its pinned image is never written again
            tab.upload(*self._build(entries))
        else:
            tab = self._eager
            if key != self._key:
                tensors, chunks = self._build(entries)
                host = torch.empty(tab.nbytes, dtype=torch.uint8).pin_memory()
                tab.upload(tensors, chunks, host)
                _RETIRED.add(host)
                self._key = key
            if self._hyper != self._hyper_values():
                self.sync_hyperparameters()
        L, st = _lib.lib(), _lib.stream_handle()
        state, part = self._block.data_ptr(), self._partials.data_ptr()
        _lib.check(L.sca_optim_grad_sqnorm(tab.tensors_ptr, tab.chunks_ptr, tab.nchunks, self.max_blocks,
                                           _lib.ptr(loss), state, part, st), "sca_optim_grad_sqnorm")
        _lib.check(L.sca_optim_adam_step(tab.tensors_ptr, tab.chunks_ptr, tab.nchunks, self._groups_dev.data_ptr(),
                                         self.max_blocks, float(self.max_grad_norm or 0.0), state, part, st),
                   "sca_optim_adam_step")
        self._calls += 1
        return out

    def _view(self, i, dtype):
        if self._block is None:
            raise RuntimeError("FusedAdam: no step() has run yet")
        return self._block.view(dtype)[i]

    @property
    def step_count(self):
        """Device int32: updates applied (skipped calls are not counted)."""
        return self._view(0, torch.int32)

    @property
    def skipped(self):
        """Device int32: 1 when the last step() saw a non-finite loss."""
        return self._view(1, torch.int32)

    @property
    def grad_norm(self):
        """Device fp32: total 2-norm of the last step's gradients, before clipping."""
        return self._view(2, torch.float32)

    @property
    def clip_coef(self):
        """Device fp32: the last step's clip coefficient (1 when clipping is off or idle)."""
        return self._view(3, torch.float32)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.Adam's format (per-parameter step, exp_avg, exp_avg_sq, max_exp_avg_sq).
        Reads the device step count (a host sync)."""
        if self._block is not None:
            self._calls = int(self._block[0].item())
            for p, st in self.state.items():
                if p in self._t0:
                    st["step"] = torch.tensor(float(max(self._calls - self._t0[p], 0)))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Load a checkpoint written by FusedAdam or by torch.optim.Adam."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for k in _UNSUPPORTED:
                if group.get(k):
                    raise TypeError(f"FusedAdam does not support {k}={group[k]!r}")
        self._capacity = None  # amsgrad may have changed with the groups
        self._ensure_device()
        steps = {p: int(float(st.get("step", 0))) for p, st in self.state.items()}
        top = max(steps.values(), default=0)
        for p, st in self.state.items():
            gi = self._slot[p][0]
            names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if self.param_groups[gi]["amsgrad"] else [])
            for name in names:
                mine = self._moment(p, name)
                if name in st:
                    mine.copy_(st[name])
                else:
                    mine.zero_()
                st[name] = mine
            st["step"] = torch.tensor(float(steps[p]))
            self._t0[p] = top - steps[p]
        self._calls = top
        self._block[:2].copy_(torch.tensor([top, 0], dtype=torch.int32))
        self._key = None
        self._hyper = None


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """Drop-in for torch.nn.utils.clip_grad_norm_ (opt.py:34) on the HIP path: scales the
    gradients in place by min(1, max_norm / (total_norm + 1e-6)) and returns the total
    2-norm as a device tensor, without a host sync."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only norm_type 2 is supported on the HIP path, got {norm_type}")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        if not g.is_cuda:
            raise RuntimeError(_NO_CPU.format(g.device, g.dtype))
        _check_tensor(g, "clip_grad_norm_ gradient")
    dev = grads[0].device
    tensors = np.zeros(len(grads), dtype=_TENSOR_DT)
    tensors["g"] = [g.data_ptr() for g in grads]
    tensors["numel"] = [g.numel() for g in grads]
    chunks = plan_chunks(tensors["numel"])
    tab = _Tables(len(tensors), len(chunks), dev)
    tab.upload(tensors, chunks)
    _RETIRED.add(tab.host)
    L, st = _lib.lib(), _lib.stream_handle()
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    part = torch.zeros(L.sca_optim_blocks(0, len(chunks)), dtype=torch.float32, device=dev)
    _lib.check(L.sca_optim_grad_sqnorm(tab.tensors_ptr, tab.chunks_ptr, tab.nchunks, 0, None, state.data_ptr(),
                                       part.data_ptr(), st), "sca_optim_grad_sqnorm")
    _lib.check(L.sca_optim_scale_grads(tab.tensors_ptr, tab.chunks_ptr, tab.nchunks, 0, float(max_norm),
                                       state.data_ptr(), part.data_ptr(), st), "sca_optim_scale_grads")
    return state.view(torch.float32)[2]


class WarmupCosineAnnealingScheduler(_LRScheduler):
    """The yaml's `warmupcosineannealing` (optimizer.py:313-359): the rate climbs linearly to
    the base rate over the first int(total_epochs * warmup_ratio) epochs, then follows half a
    cosine down to eta_min at total_epochs."""

    def __init__(self, optimizer, total_epochs, warmup_ratio=0.2, eta_min=0, last_epoch=-1):
        self.total_epochs = total_epochs
        self.warmup_epochs = int(total_epochs * warmup_ratio)
        self.eta_min = eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        epoch = self.last_epoch
        if epoch < self.warmup_epochs:
            return [base * (epoch + 1) / self.warmup_epochs for base in self.base_lrs]
        progress = (epoch - self.warmup_epochs) / (self.total_epochs - self.warmup_epochs)
        return [self.eta_min + (base - self.eta_min) * (1 + math.cos(math.pi * progress)) / 2
                for base in self.base_lrs]


_NOT_ON_HIP = ("adagrad", "adadelta", "rmsprop", "sgd")


def build_optimizer(config, model, max_grad_norm=None):
    """optimizer.py:33-66 on the HIP path: one parameter group per model child, its lr the
    `learning_rate` entry whose key is a substring of the child's name (the last match wins)
    or `learning_rate.default`; "adam" and "adamw" both give FusedAdam (plain Adam, as in the
    reference).  `config` is not modified."""
    name = str(config.get("optimizer", "adam")).lower()
    rates = dict(config["learning_rate"])
    base_lr = float(rates.pop("default"))
    groups = []
    for child_name, child in model.named_children():
        lr = base_lr
        for key, value in rates.items():
            if key in child_name:
                lr = float(value)
        groups.append({"params": list(child.parameters()), "lr": lr})
    if name in ("adam", "adamw"):
        return FusedAdam(groups, lr=base_lr, betas=tuple(config.get("betas", (0.9, 0.999))),
                         eps=config.get("eps", 1.0e-8), weight_decay=config.get("weight_decay", 0),
                         amsgrad=config.get("amsgrad", False), max_grad_norm=max_grad_norm)
    if name in _NOT_ON_HIP:
        raise ValueError(f"Optimizer {name} is not available on the HIP path (only adam / adamw are)")
    raise ValueError("Unknown optimizer {}.".format(name))
