"""DistributedOptimizer: gradient-allreduce injection into any torch optim.

Reference: horovod/torch/optimizer.py:36-342 (grad-accumulator hooks firing
async allreduce, backward_passes_per_step, tensor groups, Average via
pre/postscale, sparse allreduce) and 345-515 (_DistributedAdasumOptimizer).

MI355X-native differences:
 * hooks use torch's register_post_accumulate_grad_hook (no expand_as
   grad_acc trick needed on torch >= 2.1);
 * compression maps to a wire dtype executed inside the CDNA4 fusion pack
   kernel instead of python-side .half() round-trips;
 * averaging folds into the unpack kernel's postscale.
"""
import warnings
from contextlib import contextmanager

import torch

from horovod_amd.torch.compression import Compression
from horovod_amd.torch import mpi_ops
from horovod_amd.torch.mpi_ops import (Adasum, Average, Sum,
                                       sparse_allreduce_async, size,
                                       synchronize)
from horovod_amd.common.process_sets import global_process_set


def _split_list(xs, n):
    k, m = divmod(len(xs), n)
    return [xs[i * k + min(i, m):(i + 1) * k + min(i + 1, m)]
            for i in range(n)]


class _DistributedOptimizer(torch.optim.Optimizer):
    def __init__(self, params, named_parameters, compression,
                 backward_passes_per_step=1, op=Average,
                 gradient_predivide_factor=1.0, groups=None,
                 sparse_as_dense=False, process_set=global_process_set):
        super(self.__class__, self).__init__(params)

        self._compression = compression or Compression.none
        self.op = op
        self.gradient_predivide_factor = gradient_predivide_factor
        self.backward_passes_per_step = backward_passes_per_step
        self.sparse_as_dense = sparse_as_dense
        self.process_set = process_set

        if named_parameters is not None:
            named_parameters = list(named_parameters)
        else:
            named_parameters = [(f"allreduce.noname.{i}.{j}", v)
                                for i, group in enumerate(self.param_groups)
                                for j, v in enumerate(group["params"])]
        # check uniqueness (reference optimizer.py:67-77)
        all_names = [n for n, _ in named_parameters]
        if len(set(all_names)) < len(all_names):
            raise ValueError(
                "named_parameters has duplicate names; ensure model parameter "
                "names are unique")
        named = {v: k for k, v in named_parameters}
        self._parameter_names = {}
        for group in self.param_groups:
            for p in group["params"]:
                self._parameter_names[p] = named.get(
                    p, f"allreduce.noname.{len(self._parameter_names)}")

        self._handles = {}          # param -> handle or sparse closure
        self._grad_accs = []
        self._requires_update = set()
        self._synchronized = False
        self._should_synchronize = True
        self._allreduce_delay = {}

        # tensor groups (reference optimizer.py:88-103) --------------------
        self._groups = None
        self._p_to_group = {}
        self._group_counts = {}
        if groups is not None:
            all_params = [p for group in self.param_groups
                          for p in group["params"] if p.requires_grad]
            if isinstance(groups, int):
                grouped = _split_list(all_params, max(1, min(groups,
                                                             len(all_params))))
            else:
                grouped = [list(g) for g in groups]
            self._groups = grouped
            for gi, g in enumerate(grouped):
                for p in g:
                    self._p_to_group[p] = gi
                self._group_counts[gi] = 0

        if size() > 1 or _force_allreduce():
            self._register_hooks()

    # ------------------------------------------------------------------
    def _register_hooks(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad:
                    self._requires_update.add(p)
                    self._allreduce_delay[p] = self.backward_passes_per_step
                    acc = p.register_post_accumulate_grad_hook(
                        self._make_hook())
                    self._grad_accs.append(acc)

    def _make_hook(self):
        def hook(p):
            if p in self._handles and self._handles[p] is not None:
                if self._allreduce_delay[p] <= 0:
                    raise AssertionError(
                        "Gradients were computed more than "
                        "backward_passes_per_step times before call to "
                        "step(). Increase backward_passes_per_step.")
            self._allreduce_delay[p] -= 1
            if self._allreduce_delay[p] == 0:
                self._handles[p] = self._allreduce_grad_async(p)
        return hook

    def _allreduce_args(self):
        if self.op == Average:
            if self.gradient_predivide_factor != 1.0:
                # reference optimizer.py:197-204
                return (Sum, 1.0 / self.gradient_predivide_factor,
                        self.gradient_predivide_factor / size())
            return (Average, 1.0, 1.0)
        if self.op == Adasum:
            return (Adasum, 1.0, 1.0)
        return (self.op, 1.0, 1.0)

    def _allreduce_grad_async(self, p):
        name = self._parameter_names.get(p)
        if p.grad is None:
            # fixed-size zero gradient so the collective still matches peers
            p.grad = torch.zeros_like(p.data)
        if p.grad.is_sparse:
            if self.sparse_as_dense:
                p.grad = p.grad.to_dense()
            else:
                # a sparse-gradient param cannot ride a dense tensor group:
                # drop it from its group on first sighting so the group's
                # member count matches the hooks that will actually fire
                # (otherwise the group either never fires or fires with a
                # sparse tensor in the fused bucket)
                if self._groups is not None and p in self._p_to_group:
                    gi = self._p_to_group.pop(p)
                    self._groups[gi] = [q for q in self._groups[gi]
                                        if q is not p]
                return sparse_allreduce_async(
                    p.grad, name=name,
                    op=self.op if self.op != Average else Average,
                    process_set=self.process_set)
        op, pre, post = self._allreduce_args()
        wire = self._compression.wire_dtype(p.grad.dtype)

        if self._groups is not None:
            gi = self._p_to_group[p]
            self._group_counts[gi] += 1
            if self._group_counts[gi] == len(self._groups[gi]):
                self._group_counts[gi] = 0
                grads = [q.grad for q in self._groups[gi]]
                handle = mpi_ops._grouped_allreduce_impl(
                    grads, grads, None,
                    self._parameter_names.get(self._groups[gi][0]),
                    op, pre, post, self.process_set, wire_dtype=wire)
                for q in self._groups[gi]:
                    self._handles[q] = ("group", handle)
                return self._handles[p]
            return None  # pending group fire

        return mpi_ops._do_allreduce_async(
            p.grad, p.grad, None, name, op, pre, post, self.process_set,
            wire_dtype=wire)

    # ------------------------------------------------------------------
    def synchronize(self):
        """Wait for all outstanding gradient allreduces (reference:
        optimizer.py:255-323)."""
        # Params whose hooks never fired (per-rank conditional execution)
        # must still be submitted, or peers stall waiting on the missing
        # tensor (reference: missing_p = _requires_update - handled).
        missing = [p for p in self._requires_update if p not in self._handles]
        for p in missing:
            self._handles[p] = self._allreduce_grad_async(p)
        for p in list(self._handles.keys()):
            # re-read on every iteration: firing one group member can
            # complete the group and fill every member's handle — a stale
            # snapshot would double-fire and corrupt _group_counts
            if self._handles[p] is None:
                self._handles[p] = self._allreduce_grad_async(p)
        seen_groups = set()
        for p, handle in self._handles.items():
            if handle is None:
                continue
            if callable(handle):  # sparse closure
                p.grad = handle()
            elif isinstance(handle, tuple) and handle[0] == "group":
                if handle[1] not in seen_groups:
                    synchronize(handle[1])
                    seen_groups.add(handle[1])
            else:
                synchronize(handle)
            self._allreduce_delay[p] = self.backward_passes_per_step
        self._handles.clear()
        self._synchronized = True

    @contextmanager
    def skip_synchronize(self):
        """Use when calling synchronize() manually before step()."""
        self._should_synchronize = False
        try:
            yield
        finally:
            self._should_synchronize = True

    def step(self, closure=None):
        if self._should_synchronize:
            if self._synchronized:
                warnings.warn(
                    "optimizer.step() called without a prior backward; "
                    "calling synchronize() again")
            self.synchronize()
        self._synchronized = False
        return super(self.__class__, self).step(closure)

    def set_backward_passes_per_step(self, passes):
        """Reference: optimizer.py set_backward_passes_per_step."""
        self.backward_passes_per_step = passes
        for p in self._allreduce_delay:
            self._allreduce_delay[p] = passes

    def load_state_dict(self, *args, **kwargs):
        # dropping in a new state invalidates in-flight gradient bookkeeping
        # (reference: _DistributedOptimizer.load_state_dict)
        result = super(self.__class__, self).load_state_dict(*args, **kwargs)
        self.reset_distributed_state()
        return result

    def reset_distributed_state(self):
        """Drop in-flight allreduce bookkeeping after an elastic reset (the
        native handles died with the old controller)."""
        self._handles.clear()
        for p in self._allreduce_delay:
            self._allreduce_delay[p] = self.backward_passes_per_step
        for gi in self._group_counts:
            self._group_counts[gi] = 0
        self._synchronized = False

    def zero_grad(self, *args, **kwargs):
        if self._handles:
            raise AssertionError(
                "optimizer.zero_grad() was called after loss.backward() but "
                "before optimizer.step() or optimizer.synchronize(). This is "
                "prohibited as it can cause a race condition.")
        return super(self.__class__, self).zero_grad(*args, **kwargs)


class _DistributedAdasumOptimizer(torch.optim.Optimizer):
    """Adasum delta optimization (reference: optimizer.py:345-515): apply
    the wrapped optimizer LOCALLY, Adasum-reduce the resulting weight DELTA,
    then set w = w_start + reduced_delta.  This is the semantically correct
    way to combine Adasum with stateful optimizers (Adam etc.)."""

    def __init__(self, params, named_parameters, compression,
                 backward_passes_per_step=1,
                 process_set=global_process_set):
        super(self.__class__, self).__init__(params)
        self._compression = compression or Compression.none
        self.backward_passes_per_step = backward_passes_per_step
        self.process_set = process_set
        if named_parameters is not None:
            named = {v: k for k, v in named_parameters}
        else:
            named = {}
        self._parameter_names = {}
        for group in self.param_groups:
            for p in group["params"]:
                self._parameter_names[p] = named.get(
                    p, f"adasum.noname.{len(self._parameter_names)}")
        self._step_count = 0

    def step(self, closure=None):
        self._step_count += 1
        if self._step_count % self.backward_passes_per_step != 0:
            return None
        params = [p for group in self.param_groups for p in group["params"]
                  if p.grad is not None]
        starts = [p.detach().clone() for p in params]
        loss = super(self.__class__, self).step(closure)
        if size() == 1 and not _force_allreduce():
            return loss
        deltas = [p.detach() - s for p, s in zip(params, starts)]
        wire = self._compression.wire_dtype(deltas[0].dtype) if deltas else None
        names = [f"adasum.delta.{self._parameter_names[p]}" for p in params]
        handle = mpi_ops._allreduce_async_impl(
            deltas, deltas, names, Adasum, 1.0, 1.0,
            self.process_set.process_set_id,
            mpi_ops._dtype_code(wire) if wire else
            mpi_ops._dtype_code(deltas[0].dtype) if deltas else 5,
            kind="grouped")
        synchronize(handle)
        with torch.no_grad():
            for p, s, d in zip(params, starts, deltas):
                p.detach().copy_(s.add_(d))
        return loss

    def synchronize(self):
        pass

    @contextmanager
    def skip_synchronize(self):
        yield

    def zero_grad(self, *args, **kwargs):
        return super(self.__class__, self).zero_grad(*args, **kwargs)

    def set_backward_passes_per_step(self, passes):
        """The Adasum variant paces by _step_count modulo, not per-param
        delays (reference: optimizer.py set_backward_passes_per_step)."""
        self.backward_passes_per_step = passes

    def load_state_dict(self, *args, **kwargs):
        # dropping in a new state invalidates in-flight gradient bookkeeping
        # (reference: _DistributedOptimizer.load_state_dict)
        result = super(self.__class__, self).load_state_dict(*args, **kwargs)
        self.reset_distributed_state()
        return result

    def reset_distributed_state(self):
        pass


def _force_allreduce():
    import os
    return os.environ.get("HOROVOD_ELASTIC", "0") == "1"


def DistributedOptimizer(optimizer, named_parameters=None,
                         compression=Compression.none,
                         backward_passes_per_step=1, op=Average,
                         gradient_predivide_factor=1.0,
                         num_groups=0, groups=None, sparse_as_dense=False,
                         process_set=global_process_set):
    """Wrap a torch optimizer with distributed gradient averaging
    (reference: optimizer.py:516-608)."""
    if gradient_predivide_factor != 1.0 and op != Average:
        raise ValueError(
            "gradient_predivide_factor not supported with op != Average")
    if num_groups != 0:
        warnings.warn("Parameter `num_groups` has been replaced by `groups`",
                      DeprecationWarning)
        if groups is None:
            groups = num_groups
    if groups is not None and not isinstance(groups, (list, int)):
        raise ValueError("groups should be a list or int")

    if op == Adasum:
        # delta optimization (reference: factory optimizer.py:516+ routes
        # op=Adasum to _DistributedAdasumOptimizer)
        cls = type(optimizer.__class__.__name__, (optimizer.__class__,),
                   dict(_DistributedAdasumOptimizer.__dict__))
        return cls(optimizer.param_groups, named_parameters, compression,
                   backward_passes_per_step, process_set)

    cls = type(optimizer.__class__.__name__, (optimizer.__class__,),
               dict(_DistributedOptimizer.__dict__))
    return cls(optimizer.param_groups, named_parameters, compression,
               backward_passes_per_step, op, gradient_predivide_factor,
               groups, sparse_as_dense, process_set)
