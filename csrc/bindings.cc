// pybind11 bindings (reference: horovod/torch/mpi_ops_v2.cc N24).
//
// One templated entry point per op instead of per-dtype symbol names; the
// Python layer (horovod_amd/torch/mpi_ops.py) builds the hvd.* surface on
// top of these.
#include <torch/extension.h>

#include "core.h"
#include "timeline.h"
#include "gpu.h"

namespace {

using namespace hvd;

ReduceOp OpFromInt(int op) { return (ReduceOp)op; }

py::tuple WaitHandle(int handle) {
  std::vector<at::Tensor> outputs;
  at::Tensor extra;
  int32_t result_int = -1;
  Status s;
  {
    py::gil_scoped_release nogil;
    s = State().handles.Wait(handle, outputs, extra, &result_int);
  }
  if (!s.ok()) {
    if (s.type == StatusType::ABORTED)
      throw std::runtime_error("HorovodInternalError: " + s.reason);
    throw std::runtime_error(s.reason);
  }
  py::list outs;
  for (auto& t : outputs) outs.append(t);
  py::object extra_obj = py::none();
  if (extra.defined()) extra_obj = py::cast(extra);
  return py::make_tuple(outs, extra_obj, result_int);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "horovod_amd core (MI355X-native: TCP controller + RCCL/xGMI)";

  m.def("init",
        [](int rank, int size, int local_rank, int local_size, int cross_rank,
           int cross_size, const std::string& addr, int port,
           int64_t fusion_threshold, double cycle_time_ms, int cache_capacity,
           double stall_warning_sec, double stall_shutdown_sec, bool timeline) {
          ControllerConfig cfg;
          cfg.fusion_threshold_bytes = fusion_threshold;
          cfg.cycle_time_ms = cycle_time_ms;
          cfg.cache_capacity = (size_t)cache_capacity;
          cfg.stall_warning_sec = stall_warning_sec;
          cfg.stall_shutdown_sec = stall_shutdown_sec;
          cfg.timeline_enabled = timeline;
          py::gil_scoped_release nogil;
          InitHorovod(rank, size, local_rank, local_size, cross_rank, cross_size,
                      addr, port, cfg);
        },
        py::arg("rank"), py::arg("size"), py::arg("local_rank"),
        py::arg("local_size"), py::arg("cross_rank"), py::arg("cross_size"),
        py::arg("addr"), py::arg("port"), py::arg("fusion_threshold"),
        py::arg("cycle_time_ms"), py::arg("cache_capacity"),
        py::arg("stall_warning_sec"), py::arg("stall_shutdown_sec"),
        py::arg("timeline"));

  m.def("interrupt", [](const std::string& why) {
    py::gil_scoped_release nogil;
    InterruptHorovod(why);
  });
  m.def("shutdown", [] {
    py::gil_scoped_release nogil;
    ShutdownHorovod();
  });
  m.def("is_initialized", &IsInitialized);

  m.def("rank", [] { return State().rank; });
  m.def("size", [] { return State().size; });
  m.def("local_rank", [] { return State().local_rank; });
  m.def("local_size", [] { return State().local_size; });
  m.def("cross_rank", [] { return State().cross_rank; });
  m.def("cross_size", [] { return State().cross_size; });
  m.def("rccl_used", [] { return hvd::gpu::RcclUsed(); });

  m.def("set_fusion_threshold",
        [](int64_t b) { if (State().controller) State().controller->set_fusion_threshold(b); });
  m.def("get_fusion_threshold",
        [] { return State().controller ? State().controller->fusion_threshold() : 0; });
  m.def("set_cycle_time_ms",
        [](double ms) { if (State().controller) State().controller->set_cycle_time_ms(ms); });
  m.def("get_cycle_time_ms",
        [] { return State().controller ? State().controller->cycle_time_ms() : 0.0; });

  // ---- enqueue ops --------------------------------------------------------
  m.def("allreduce_async",
        [](std::vector<at::Tensor> tensors, std::vector<at::Tensor> outputs,
           std::vector<std::string> names, int op, double prescale,
           double postscale, int process_set, int wire_dtype) {
          return EnqueueAllreduceMulti(std::move(tensors), std::move(outputs),
                                       std::move(names), OpFromInt(op), prescale,
                                       postscale, process_set,
                                       (DataType)wire_dtype);
        });
  m.def("allgather_async", [](at::Tensor t, const std::string& name, int ps) {
    return EnqueueAllgather(t, name, ps);
  });
  m.def("broadcast_async",
        [](at::Tensor t, at::Tensor out, int root, const std::string& name,
           int ps) { return EnqueueBroadcast(t, out, root, name, ps); });
  m.def("alltoall_async",
        [](at::Tensor t, at::Tensor splits, const std::string& name, int ps) {
          return EnqueueAlltoall(t, splits, name, ps);
        });
  m.def("reducescatter_async",
        [](at::Tensor t, const std::string& name, int op, double prescale,
           double postscale, int ps) {
          return EnqueueReducescatter(t, name, OpFromInt(op), prescale, postscale,
                                      ps);
        });
  m.def("join_async", [](int device, int ps) { return EnqueueJoin(device, ps); });
  m.def("barrier_async", [](int ps) { return EnqueueBarrier(ps); });

  // ---- completion ---------------------------------------------------------
  m.def("poll", [](int handle) { return State().handles.Poll(handle); });
  m.def("flush", [] { FlushCycle(); });
  m.def("wait", &WaitHandle);

  m.def("adasum_combine_", [](std::vector<at::Tensor> a,
                              std::vector<at::Tensor> b) {
    hvd::gpu::AdasumCombine(a, b);
  });

  // ---- global-norm gradient clipping ------------------------------------
  m.def("multi_tensor_grad_norm",
        [](std::vector<at::Tensor> grads, double max_norm) {
          return hvd::gpu::MultiTensorGradNorm(grads, max_norm);
        },
        py::arg("grads"), py::arg("max_norm"));
  auto opt_tensor = [](const py::object& o) {
    return o.is_none() ? at::Tensor() : o.cast<at::Tensor>();
  };
  // the norm pass of a loss-scaled step -> {total_norm, coef, found, scale}
  m.def("multi_tensor_scaled_grad_norm",
        [opt_tensor](std::vector<at::Tensor> grads,
                     std::optional<double> max_norm, py::object scale,
                     py::object found_inf, py::object growth_tracker,
                     double growth_factor, double backoff_factor,
                     int64_t growth_interval) {
          return hvd::gpu::MultiTensorScaledGradNorm(
              grads, max_norm, opt_tensor(scale), opt_tensor(found_inf),
              opt_tensor(growth_tracker), growth_factor, backoff_factor,
              growth_interval);
        },
        py::arg("grads"), py::arg("max_norm") = py::none(),
        py::arg("scale") = py::none(), py::arg("found_inf") = py::none(),
        py::arg("growth_tracker") = py::none(),
        py::arg("growth_factor") = 1.0, py::arg("backoff_factor") = 1.0,
        py::arg("growth_interval") = 0);
  m.def("multi_tensor_scale_",
        [](std::vector<at::Tensor> tensors, at::Tensor coef) {
          hvd::gpu::MultiTensorScale(tensors, coef);
        },
        py::arg("tensors"), py::arg("coef"));

  // ---- fused optimizer kernels (grad_coef: None or a 1-element fp32
  // device tensor, e.g. multi_tensor_grad_norm(...)[1:2]; skip: None or such
  // a tensor that, nonzero, turns the call into a no-op on the device, e.g.
  // multi_tensor_scaled_grad_norm(...)[2:3]) --------------------------------
  // model_params: None, or the fp16/bf16 model parameters of a master-weight
  // step (params are then their fp32 masters)
  using OptTensors = std::optional<std::vector<at::Tensor>>;
  auto opt_list = [](const OptTensors& o) { return o ? &*o : nullptr; };
  m.def("fused_sgd_step",
        [opt_tensor, opt_list](std::vector<at::Tensor> params,
                     std::vector<at::Tensor> grads,
                     std::vector<at::Tensor> momenta, double lr,
                     double momentum, double weight_decay, double dampening,
                     bool nesterov, py::object grad_coef,
                     OptTensors model_params, py::object skip) {
          hvd::gpu::FusedSgdStep(params, grads, momenta, lr, momentum,
                                 weight_decay, dampening, nesterov,
                                 opt_tensor(grad_coef),
                                 opt_list(model_params), opt_tensor(skip));
        },
        py::arg("params"), py::arg("grads"), py::arg("momenta"),
        py::arg("lr"), py::arg("momentum"), py::arg("weight_decay"),
        py::arg("dampening"), py::arg("nesterov"),
        py::arg("grad_coef") = py::none(),
        py::arg("model_params") = py::none(), py::arg("skip") = py::none());

  m.def("fused_adamw_step",
        [opt_tensor, opt_list](std::vector<at::Tensor> params,
                     std::vector<at::Tensor> grads,
                     std::vector<at::Tensor> exp_avgs,
                     std::vector<at::Tensor> exp_avg_sqs, double lr,
                     double beta1, double beta2, double eps,
                     double weight_decay, int64_t step,
                     py::object grad_coef, OptTensors model_params,
                     py::object skip) {
          hvd::gpu::FusedAdamwStep(params, grads, exp_avgs, exp_avg_sqs, lr,
                                   beta1, beta2, eps, weight_decay, step,
                                   opt_tensor(grad_coef),
                                   opt_list(model_params), opt_tensor(skip));
        },
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("step"), py::arg("grad_coef") = py::none(),
        py::arg("model_params") = py::none(), py::arg("skip") = py::none());

  m.def("fused_lamb_step",
        [opt_tensor, opt_list](std::vector<at::Tensor> params,
                     std::vector<at::Tensor> grads,
                     std::vector<at::Tensor> exp_avgs,
                     std::vector<at::Tensor> exp_avg_sqs, double lr,
                     double beta1, double beta2, double eps,
                     double weight_decay, int64_t step, bool bias_correction,
                     bool adapt, py::object grad_coef,
                     OptTensors model_params, py::object skip) {
          return hvd::gpu::FusedLambStep(params, grads, exp_avgs, exp_avg_sqs,
                                         lr, beta1, beta2, eps, weight_decay,
                                         step, bias_correction, adapt,
                                         opt_tensor(grad_coef),
                                         opt_list(model_params),
                                         opt_tensor(skip));
        },
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("step"), py::arg("bias_correction"), py::arg("adapt"),
        py::arg("grad_coef") = py::none(),
        py::arg("model_params") = py::none(), py::arg("skip") = py::none());

  // -> the fp32 trust ratio of every parameter, in input order
  m.def("fused_lars_step",
        [opt_tensor, opt_list](std::vector<at::Tensor> params,
                     std::vector<at::Tensor> grads,
                     std::vector<at::Tensor> momenta, double lr,
                     double momentum, double weight_decay,
                     double trust_coefficient, double eps, bool nesterov,
                     bool trust_clip, bool adapt, py::object grad_coef,
                     OptTensors model_params, py::object skip) {
          return hvd::gpu::FusedLarsStep(params, grads, momenta, lr, momentum,
                                         weight_decay, trust_coefficient, eps,
                                         nesterov, trust_clip, adapt,
                                         opt_tensor(grad_coef),
                                         opt_list(model_params),
                                         opt_tensor(skip));
        },
        py::arg("params"), py::arg("grads"), py::arg("momenta"),
        py::arg("lr"), py::arg("momentum"), py::arg("weight_decay"),
        py::arg("trust_coefficient"), py::arg("eps"), py::arg("nesterov"),
        py::arg("trust_clip"), py::arg("adapt"),
        py::arg("grad_coef") = py::none(),
        py::arg("model_params") = py::none(), py::arg("skip") = py::none());

  m.def("fused_bn_relu_forward",
        [](at::Tensor x, py::object residual, at::Tensor gamma, at::Tensor beta,
           at::Tensor rm, at::Tensor rv, double momentum, double eps) {
          at::Tensor res;
          if (!residual.is_none()) res = residual.cast<at::Tensor>();
          return hvd::gpu::FusedBnReluForward(x, res, gamma, beta, rm, rv,
                                              momentum, eps);
        });
  // y may be None where beta is given (see FusedBnReluBackward)
  m.def("fused_bn_relu_backward",
        [](at::Tensor x, py::object y, at::Tensor dy, at::Tensor mean,
           at::Tensor invstd, at::Tensor gamma, bool need_res,
           py::object beta) {
          auto opt = [](const py::object& o) {
            return o.is_none() ? at::Tensor() : o.cast<at::Tensor>();
          };
          return hvd::gpu::FusedBnReluBackward(x, opt(y), dy, mean, invstd,
                                               gamma, need_res, opt(beta));
        },
        py::arg("x"), py::arg("y"), py::arg("dy"), py::arg("mean"),
        py::arg("invstd"), py::arg("gamma"), py::arg("need_residual_grad"),
        py::arg("beta") = py::none());
  m.def("fused_bn_lean_path", []() { return hvd::gpu::FusedBnLeanPath(); });
  m.def("fused_bn_pass",
        [](int which, at::Tensor x, py::object a, py::object b, py::object out,
           at::Tensor mean, at::Tensor invstd, at::Tensor gamma,
           at::Tensor beta) {
          auto opt = [](const py::object& o) {
            return o.is_none() ? at::Tensor() : o.cast<at::Tensor>();
          };
          hvd::gpu::FusedBnPass(which, x, opt(a), opt(b), opt(out), mean,
                                invstd, gamma, beta);
        });

  // ---- fused dropout + add + LayerNorm (None = absent optional tensor) -----
  // -> [y, z|None, mean, rstd]
  m.def("fused_ln_forward",
        [opt_tensor](at::Tensor x, py::object residual, py::object weight,
                     py::object bias, double p, double eps, uint64_t seed,
                     uint64_t offset, bool save_z) {
          return hvd::gpu::FusedLnForward(x, opt_tensor(residual),
                                          opt_tensor(weight), opt_tensor(bias),
                                          p, eps, seed, offset, save_z);
        },
        py::arg("x"), py::arg("residual"), py::arg("weight"), py::arg("bias"),
        py::arg("p"), py::arg("eps"), py::arg("seed"), py::arg("offset"),
        py::arg("save_z"));
  // -> [dz, dx, dgamma|None, dbeta|None]
  m.def("fused_ln_backward",
        [opt_tensor](at::Tensor dy, at::Tensor z, at::Tensor mean,
                     at::Tensor rstd, py::object weight, double p,
                     uint64_t seed, uint64_t offset, bool need_wgrad) {
          return hvd::gpu::FusedLnBackward(dy, z, mean, rstd,
                                           opt_tensor(weight), p, seed, offset,
                                           need_wgrad);
        },
        py::arg("dy"), py::arg("z"), py::arg("mean"), py::arg("rstd"),
        py::arg("weight"), py::arg("p"), py::arg("seed"), py::arg("offset"),
        py::arg("need_wgrad"));
  // device: a torch.device or its string
  m.def("fused_ln_keep_mask",
        [](int64_t rows, int64_t H, double p, uint64_t seed, uint64_t offset,
           py::object device) {
          return hvd::gpu::FusedLnKeepMask(
              rows, H, p, seed, offset,
              c10::Device(py::str(device).cast<std::string>()));
        },
        py::arg("rows"), py::arg("H"), py::arg("p"), py::arg("seed"),
        py::arg("offset"), py::arg("device"));

  // ---- SyncBatchNorm passes (None = absent optional tensor) ----------------
  m.def("sync_bn_stats",
        [](at::Tensor x) { return hvd::gpu::SyncBnStats(x); });
  m.def("sync_bn_normalize",
        [](at::Tensor x, at::Tensor stats, py::object weight, py::object bias,
           py::object rm, py::object rv, double momentum, double eps) {
          auto opt = [](const py::object& o) {
            return o.is_none() ? at::Tensor() : o.cast<at::Tensor>();
          };
          return hvd::gpu::SyncBnNormalize(x, stats, opt(weight), opt(bias),
                                           opt(rm), opt(rv), momentum, eps);
        });
  m.def("sync_bn_backward_reduce",
        [](at::Tensor x, at::Tensor dy, at::Tensor mean, at::Tensor invstd) {
          return hvd::gpu::SyncBnBackwardReduce(x, dy, mean, invstd);
        });
  m.def("sync_bn_backward_apply",
        [](at::Tensor x, at::Tensor dy, at::Tensor mean, at::Tensor invstd,
           py::object weight, at::Tensor sums, at::Tensor count) {
          at::Tensor w;
          if (!weight.is_none()) w = weight.cast<at::Tensor>();
          return hvd::gpu::SyncBnBackwardApply(x, dy, mean, invstd, w, sums,
                                               count);
        });

  // ---- timeline -----------------------------------------------------------
  m.def("start_timeline", [](const std::string& path, bool mark_cycles) {
    auto& st = State();
    if (!st.initialized) throw std::runtime_error("not initialized");
    SetTimeline(st, std::make_shared<Timeline>(path, st.rank));
    (void)mark_cycles;
  });
  m.def("stop_timeline", [] {
    auto tl = GetTimeline(State());
    SetTimeline(State(), nullptr);
    if (tl) {
      py::gil_scoped_release nogil;
      tl->Finalize();  // file is complete, valid JSON on return
    }
  });

  // ---- process sets -------------------------------------------------------
  m.def("add_process_set", [](std::vector<int32_t> ranks) {
    if (!State().controller) throw std::runtime_error("not initialized");
    return State().controller->AddProcessSet(ranks);
  });
  m.def("remove_process_set", [](int id) {
    if (State().controller) State().controller->RemoveProcessSet(id);
  });
  m.def("process_set_ranks", [](int id) {
    if (!State().controller || !State().controller->has_process_set(id))
      throw std::runtime_error("unknown process set");
    return State().controller->process_set(id).ranks;
  });
}
