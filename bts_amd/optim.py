"""``NativeAdamW``: the training step's optimiser on libbts_hip.so (csrc/optim.hip, bts_adamw_step_f32).

One launch updates every parameter that has a gradient and, for the dense 1x1 / 3x3 convolution weights registered with
the training step's ``WeightPacker``, writes the new values straight into the packed forward / input-gradient buffers the
convolution kernels read.  Same constructor arguments, param-group keys and per-parameter state
(``state[p] = {'step', 'exp_avg', 'exp_avg_sq'}``, ``step`` a CPU float tensor) as ``torch.optim.AdamW``: the base class's
``state_dict()`` / ``load_state_dict()`` work unchanged and a checkpoint written by either optimiser loads into the other.

There is no CPU path: ``step()`` on a parameter that does not live on a GPU raises ``BtsHipError``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import BtsHipError

MAX_HYPER = 8          # hyper-parameter records one launch takes by value (include/bts_hip.h)


class NativeAdamW(torch.optim.Optimizer):
    """AdamW (amsgrad=False, maximize=False) as one HIP launch per step; see the module docstring.

    ``step(skip=t)``: ``t`` is a one-element float32 tensor on the parameters' device; when it is non-zero or NaN the
    launch leaves parameters, state and packs untouched (the host never reads it: no synchronisation).  The per-parameter
    ``step`` counters advance either way -- the host cannot know -- so a skipped step still ages the bias corrections.

    After a step ``attached`` lists the WeightPacker entries the launch re-packed and ``unattached`` the entries of updated
    weights that stay with the pack launch (grouped weights, the 7x7 stem, a weight packed under two strides);
    ``uploads`` counts table uploads (0 in steady state: the device table is re-sent only when a pointer or a hyper index
    moved) and ``launches`` the launches of the last step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= float(lr):
            raise ValueError("Invalid learning rate: %s" % lr)
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %s" % eps)
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: %s" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % weight_decay)
        if amsgrad or maximize or capturable or differentiable or fused:
            raise ValueError("NativeAdamW implements amsgrad=False, maximize=False, capturable=False, differentiable=False, "
                             "fused in (None, False): the update is one native launch already")
        # the keys torch.optim.AdamW keeps in a param group, so that either optimiser can load the other's state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=foreach, capturable=False, differentiable=False, fused=fused, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self.uploads = 0
        self.launches = 0
        self.attached: List[dict] = []
        self.unattached: List[dict] = []
        self._cache = None
        self._staging = []                 # [pinned tensor, event of its last copy]

    def __setstate__(self, state):
        super().__setstate__(state)
        self._cache = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # a checkpoint of torch's fused / capturable AdamW keeps `step` on the device: here it lives on the host
        for st in self.state.values():
            s = st.get("step")
            if isinstance(s, torch.Tensor) and s.device.type != "cpu":
                st["step"] = s.detach().to("cpu", torch.float32)
        self._cache = None                 # new state tensors: rebuild the table

    # ------------------------------------------------------------------------------------------------------ the table
    def _stage(self, nbytes: int) -> torch.Tensor:
        """Pinned host memory that no copy in flight still reads (event query, never a device sync)."""
        for slot in self._staging:
            if slot[0].numel() >= nbytes and (slot[1] is None or slot[1].query()):
                return slot[0]
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        self._staging.append([buf, None])
        return buf

    def _upload(self, host: np.ndarray, dev: torch.Tensor):
        buf = self._stage(host.nbytes)
        buf[:host.nbytes].numpy()[:] = host
        dev.copy_(buf[:host.nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev.device))
        for slot in self._staging:
            if slot[0] is buf:
                slot[1] = ev
        self.uploads += 1

    def _build(self, active, packer):
        """Item list for the parameters that have a gradient: geometry and pack destinations (pointers come per step)."""
        by_weight = {}
        for key, e in packer.entries.items():
            w = e["wref"]()
            if w is not None:
                by_weight.setdefault(id(w), []).append((key, e))
        items = np.zeros(len(active), dtype=np.dtype(_lib.AdamwItem))
        attached, unattached, item_entries = [], [], []
        for i, (p, _gi) in enumerate(active):
            items["numel"][i] = p.numel()
            ents = by_weight.get(id(p), [])
            modes = [key[3] for key, _ in ents]
            ok = (bool(ents) and p.dim() == 4 and p.shape[2] == p.shape[3] and p.shape[2] in (1, 3)
                  and all(key[4] == 1 and key[1] == tuple(p.shape) and e["version"] != -1 and len(e["rows"]) == 1
                          for key, e in ents)
                  and len(modes) == len(set(modes)) and len(ents) <= 2)
            mine = []
            if ok:
                items["c_out"][i], items["c_in"][i], items["ksize"][i] = p.shape[0], p.shape[1], p.shape[2]
                items["n_packs"][i] = len(ents)
                for k, (key, e) in enumerate(ents):
                    row = e["rows"][0]
                    items["packs"]["dst"][i, k] = e["dst"].data_ptr()
                    items["packs"]["k_pad"][i, k] = row[7]
                    items["packs"]["c_in_ld"][i, k] = row[5]
                    items["packs"]["mode"][i, k] = key[3]
                    mine.append(e)
                attached.extend(mine)
            else:
                unattached.extend(e for _, e in ents)
            item_entries.append(mine)
        return dict(items=items, attached=attached, unattached=unattached, item_entries=item_entries,
                    ptrs=None, launches=[])

    def _plan_launches(self, cache, ptrs, q, device):
        """(Re)fill the host tables from the current pointers and hyper indices and send them to the device."""
        lib = _lib.load_real()
        items = cache["items"]
        items["p"], items["g"], items["m"], items["v"] = ptrs[:, 0], ptrs[:, 1], ptrs[:, 2], ptrs[:, 3]
        items["hyper"] = q % MAX_HYPER
        launches = []
        old = cache["launches"]
        for li in range(int(q.max()) // MAX_HYPER + 1):
            sub = np.ascontiguousarray(items[(q // MAX_HYPER) == li])
            n = len(sub)
            if n == 0:
                launches.append(None)
                continue
            host = np.zeros(int(lib.bts_adamw_table_bytes(n)), dtype=np.uint8)
            total = C.c_long(0)
            _lib.check(lib.bts_adamw_plan_f32(sub.ctypes.data, n, host.ctypes.data, C.byref(total), None), "bts_adamw_plan_f32")
            dev = old[li]["dev"] if li < len(old) and old[li] is not None and old[li]["dev"].numel() == host.nbytes else \
                torch.empty(host.nbytes, dtype=torch.uint8, device=device)
            self._upload(host, dev)
            launches.append(dict(n=n, blocks=int(total.value), dev=dev, first_pair=li * MAX_HYPER))
        cache["launches"] = launches
        cache["ptrs"], cache["q"] = ptrs.copy(), q.copy()

    # ----------------------------------------------------------------------------------------------------------- step
    @torch.no_grad()
    def step(self, closure=None, skip: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import ops, train, workspace
        packer = train._PACKER
        found, device = [], None
        for gi, group in enumerate(self.param_groups):              # every check comes before the first change of state
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda:
                    raise BtsHipError("NativeAdamW.step: parameter on %s -- the native optimiser runs on the GPU only "
                                      "(there is no CPU fallback); use torch.optim.AdamW for CPU parameters" % p.device)
                if g.is_sparse:
                    raise RuntimeError("NativeAdamW does not support sparse gradients")
                if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous():
                    raise BtsHipError("NativeAdamW.step: parameters and gradients must be contiguous float32")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise BtsHipError("NativeAdamW.step: all parameters of one optimiser must live on one device")
                if g.device != device:
                    raise BtsHipError("NativeAdamW.step: gradient on %s, parameter on %s" % (g.device, device))
                found.append((p, gi, g if g.is_contiguous() else g.contiguous()))
        if not found:
            return loss
        if skip is not None:
            if not (isinstance(skip, torch.Tensor) and skip.device == device and skip.dtype == torch.float32 and skip.numel() == 1):
                raise BtsHipError("NativeAdamW.step: skip must be a one-element float32 tensor on %s" % device)
        active, grads, pairs, pair_of = [], [], [], {}
        for p, gi, g in found:
            st = self.state[p]
            if len(st) == 0:                                        # lazily, as torch.optim.AdamW does
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["step"] += 1
            key = (gi, float(st["step"]))                           # one hyper record per distinct (group, step count)
            qi = pair_of.get(key)
            if qi is None:
                qi = pair_of[key] = len(pairs)
                pairs.append(key)
            active.append((p, gi, qi))
            grads.append(g)
        ckey = (tuple(id(p) for p, _, _ in active), len(packer.entries), packer.epoch)
        cache = self._cache
        if cache is None or cache["key"] != ckey:
            cache = self._cache = self._build([(p, gi) for p, gi, _ in active], packer)
            cache["key"] = ckey
        ptrs = np.empty((len(active), 4), dtype=np.uint64)
        for i, ((p, _, _), g) in enumerate(zip(active, grads)):
            st = self.state[p]
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if m.device != device or v.device != device or not m.is_contiguous() or not v.is_contiguous():
                raise BtsHipError("NativeAdamW.step: exp_avg / exp_avg_sq must be contiguous tensors on %s" % device)
            ptrs[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
        q = np.fromiter((qi for _, _, qi in active), dtype=np.int64, count=len(active))
        with torch.cuda.device(device):
            if cache["ptrs"] is None or not np.array_equal(cache["ptrs"], ptrs) or not np.array_equal(cache["q"], q):
                self._plan_launches(cache, ptrs, q, device)
            skip_ptr = skip.data_ptr() if skip is not None else None
            self.launches = 0
            for L in cache["launches"]:
                if L is None:
                    continue
                sel = pairs[L["first_pair"]:L["first_pair"] + MAX_HYPER]
                hy = (_lib.AdamwHyper * len(sel))()
                for k, (gi, stepv) in enumerate(sel):
                    grp = self.param_groups[gi]
                    hy[k].lr, hy[k].beta1, hy[k].beta2 = float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1])
                    hy[k].eps, hy[k].weight_decay, hy[k].step = float(grp["eps"]), float(grp["weight_decay"]), stepv
                ops._enqueue("bts_adamw_step_f32", L["dev"], (L["dev"].data_ptr(), L["n"], L["blocks"], C.addressof(hy), len(sel), skip_ptr),
                             trace=("adamw_step_kernel", "optim.adamw", 0.0, 28.0 * int(cache["items"]["numel"].sum()), None))
                self.launches += 1
        # the kernel wrote through raw pointers: tell autograd, the packer and the eval-mode packs
        before = [p._version for p, _, _ in active]
        torch.autograd.graph.increment_version([p for p, _, _ in active])
        for (p, _, _), was, ents in zip(active, before, cache["item_entries"]):
            for e in ents:
                if skip is None or e["version"] == was:        # a skipped launch leaves a stale pack stale
                    e["version"] = p._version
                e["dst"]._bts_pack_seq = getattr(e["dst"], "_bts_pack_seq", 0) + 1
        self.attached, self.unattached = cache["attached"], cache["unattached"]
        workspace.invalidate_packs()
        packer.versions_trusted = True
        return loss
