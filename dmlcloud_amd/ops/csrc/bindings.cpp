// Python bindings for the dmlcloud_amd gfx950 kernels.
//
// This TU is compiled by the host compiler; all kernel launchers live in
// the .hip TUs and are declared here.

#include <torch/extension.h>

namespace dmlamd {

// reduce.hip
void metric_reduce_into(at::Tensor value, at::Tensor acc, at::Tensor count, at::Tensor partials,
                        int64_t op);
void metric_accumulate_elementwise(at::Tensor value, at::Tensor acc, at::Tensor count,
                                   int64_t op);
at::Tensor metric_finalize_dims(at::Tensor acc, std::vector<int64_t> dims, int64_t op);

// copy.hip
void chunked_copy(at::Tensor units_blob, int64_t nunits);

// optim.hip
void fused_adam(at::Tensor param, at::Tensor grad, at::Tensor exp_avg, at::Tensor exp_avg_sq,
                at::Tensor step_t, double lr, double beta1, double beta2, double eps,
                double weight_decay, double grad_scale);
void fused_sgd(at::Tensor param, at::Tensor grad, at::Tensor momentum_buf, double lr,
               double momentum, double weight_decay, double grad_scale, bool use_momentum);
void fused_adam_bf16(at::Tensor param, at::Tensor grad, at::Tensor master, at::Tensor exp_avg,
                     at::Tensor exp_avg_sq, at::Tensor step_t, double lr, double beta1,
                     double beta2, double eps, double weight_decay, double grad_scale);
void fused_sgd_bf16(at::Tensor param, at::Tensor grad, at::Tensor master,
                    at::Tensor momentum_buf, double lr, double momentum, double weight_decay,
                    double grad_scale, bool use_momentum);
void fused_adamw_grouped(at::Tensor param, at::Tensor grad, at::Tensor exp_avg,
                         at::Tensor exp_avg_sq, at::Tensor step_t, at::Tensor group_map,
                         at::Tensor hyper, at::Tensor sched, at::Tensor derived,
                         at::Tensor last_lr, double grad_scale);
void fused_adamw_grouped_bf16(at::Tensor param, at::Tensor grad, at::Tensor master,
                              at::Tensor exp_avg, at::Tensor exp_avg_sq, at::Tensor step_t,
                              at::Tensor group_map, at::Tensor hyper, at::Tensor sched,
                              at::Tensor derived, at::Tensor last_lr, double grad_scale);
void l2_norm_and_scale(at::Tensor flat, at::Tensor partials, at::Tensor out, double max_norm,
                       bool apply, double norm_scale);

// smallcnn.hip
void conv3x3_relu_pool_fwd(at::Tensor in, at::Tensor w, at::Tensor b, at::Tensor out,
                           at::Tensor argmax);
void conv3x3_relu_pool_bwd_data(at::Tensor dpooled, at::Tensor argmax, at::Tensor w,
                                at::Tensor din);
void conv3x3_relu_pool_bwd_weight(at::Tensor dpooled, at::Tensor argmax, at::Tensor in,
                                  at::Tensor dw, at::Tensor db);
void conv3x3_relu_pool_bwd_data_weight(at::Tensor dpooled2, at::Tensor argmax2, at::Tensor w2,
                                       at::Tensor argmax1, at::Tensor x, at::Tensor dw1,
                                       at::Tensor db1);

// layernorm.hip
void layernorm_fwd(at::Tensor x, at::Tensor gamma, at::Tensor beta, at::Tensor y,
                   at::Tensor mean, at::Tensor rstd, double eps);
void layernorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor mean, at::Tensor rstd,
                   at::Tensor gamma, at::Tensor dx, at::Tensor dgb_ws, at::Tensor dgamma,
                   at::Tensor dbeta);

// loss.hip
void ce_fwd(at::Tensor logits, at::Tensor targets, at::Tensor loss, at::Tensor lse,
            int64_t ignore_index);
void ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse, at::Tensor scale,
            at::Tensor dlogits, int64_t ignore_index);

// attention.hip
void attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse,
              double scale, bool causal, c10::optional<at::Tensor> doc_start);
void attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor dout, at::Tensor o,
              at::Tensor lse, at::Tensor dq, at::Tensor dk, at::Tensor dv, at::Tensor delta,
              double scale, bool causal, c10::optional<at::Tensor> doc_start);
void attn_decode(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor kv_len, at::Tensor o,
                 at::Tensor lse, at::Tensor ws, double scale, bool causal, int64_t num_splits);
int64_t attn_decode_workspace_floats(int64_t B, int64_t Hkv, int64_t S);
int64_t attn_decode_splits(int64_t B, int64_t Hkv, int64_t Nmax, int64_t num_splits,
                           int64_t device);
void attn_decode_tiled(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor kv_len, at::Tensor o,
                       at::Tensor lse, at::Tensor ws, double scale, bool causal,
                       int64_t num_splits, c10::optional<at::Tensor> block_table);
void kvcache_append(at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache, at::Tensor v_cache,
                    at::Tensor kv_len, c10::optional<at::Tensor> block_table);
int64_t attn_decode_tiled_workspace_floats(int64_t B, int64_t Hkv, int64_t R, int64_t S,
                                           int64_t D);
int64_t attn_decode_tiled_splits(int64_t B, int64_t Hkv, int64_t R, int64_t Nmax,
                                 int64_t num_splits, int64_t device);
void attn_decode_fp8(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor kv_len, at::Tensor o,
                     at::Tensor lse, at::Tensor ws, double scale, bool causal, int64_t num_splits,
                     c10::optional<at::Tensor> k_scale, c10::optional<at::Tensor> v_scale,
                     c10::optional<at::Tensor> block_table);
void kvcache_append_fp8(at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache, at::Tensor v_cache,
                        at::Tensor kv_len, c10::optional<at::Tensor> k_scale,
                        c10::optional<at::Tensor> v_scale, c10::optional<at::Tensor> block_table);

} // namespace dmlamd

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "dmlcloud_amd gfx950 (MI355X/CDNA4) kernels";
  m.def("metric_reduce_into", &dmlamd::metric_reduce_into,
        "Fully reduce value into scalar accumulator (deterministic)");
  m.def("metric_accumulate_elementwise", &dmlamd::metric_accumulate_elementwise,
        "Elementwise merge value into accumulator");
  m.def("metric_finalize_dims", &dmlamd::metric_finalize_dims,
        "Reduce accumulator over given dims");
  m.def("chunked_copy", &dmlamd::chunked_copy, "Descriptor-table gather/scatter copy");
  m.def("fused_adam", &dmlamd::fused_adam, "Fused Adam on flat fp32 buffers");
  m.def("fused_sgd", &dmlamd::fused_sgd, "Fused SGD on flat fp32 buffers");
  m.def("fused_adam_bf16", &dmlamd::fused_adam_bf16,
        "Fused Adam: bf16 params/grads, fp32 master + moments");
  m.def("fused_sgd_bf16", &dmlamd::fused_sgd_bf16,
        "Fused SGD: bf16 params/grads, fp32 master");
  m.def("fused_adamw_grouped", &dmlamd::fused_adamw_grouped,
        "Fused grouped AdamW on flat fp32 buffers, device-resident LR schedule");
  m.def("fused_adamw_grouped_bf16", &dmlamd::fused_adamw_grouped_bf16,
        "Fused grouped AdamW: bf16 params/grads, fp32 master + moments");
  m.def("l2_norm_and_scale", &dmlamd::l2_norm_and_scale,
        "Deterministic L2 norm + optional clip scale");
  m.def("conv3x3_relu_pool_fwd", &dmlamd::conv3x3_relu_pool_fwd,
        "Fused conv3x3(pad1)+ReLU+maxpool2x2 forward");
  m.def("conv3x3_relu_pool_bwd_data", &dmlamd::conv3x3_relu_pool_bwd_data,
        "Fused conv+relu+pool input gradient");
  m.def("conv3x3_relu_pool_bwd_weight", &dmlamd::conv3x3_relu_pool_bwd_weight,
        "Fused conv+relu+pool weight/bias gradient");
  m.def("conv3x3_relu_pool_bwd_data_weight", &dmlamd::conv3x3_relu_pool_bwd_data_weight,
        "Layer-2 input gradient and layer-1 weight/bias gradient of a two-layer "
        "conv+relu+pool stack in one kernel (no din tensor)");
  m.def("layernorm_fwd", &dmlamd::layernorm_fwd, "Fused bf16 LayerNorm forward (row per wave)");
  m.def("layernorm_bwd", &dmlamd::layernorm_bwd,
        "Fused bf16 LayerNorm backward (dx + dgamma/dbeta)");
  m.def("ce_fwd", &dmlamd::ce_fwd, "Online softmax cross-entropy forward (per-row loss + lse)");
  m.def("ce_bwd", &dmlamd::ce_bwd, "Cross-entropy backward (dlogits in one pass)");
  // doc_start is optional and trailing: the 7- and 12-argument positional
  // calls keep working
  m.def("attn_fwd", &dmlamd::attn_fwd,
        "Flash-attention forward (MFMA bf16, D=64, emits lse; optional "
        "int32 doc_start[B, N] packs several documents per row)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"), py::arg("scale"),
        py::arg("causal"), py::arg("doc_start") = py::none());
  m.def("attn_bwd", &dmlamd::attn_bwd,
        "Flash-attention backward (recompute; dq/dk/dv; optional doc_start)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dout"), py::arg("o"), py::arg("lse"),
        py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("delta"), py::arg("scale"),
        py::arg("causal"), py::arg("doc_start") = py::none());
  m.def("attn_decode", &dmlamd::attn_decode,
        "Split-KV decode attention over a K/V cache with device-resident int32 kv_len[B] "
        "(MFMA bf16, D=64, (H/Hkv)*Nq <= 16; num_splits 0 = auto)",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_len"), py::arg("o"),
        py::arg("lse"), py::arg("ws"), py::arg("scale"), py::arg("causal"), py::arg("num_splits"));
  m.def("attn_decode_workspace_floats", &dmlamd::attn_decode_workspace_floats,
        "fp32 elements attn_decode's workspace needs for S splits", py::arg("B"), py::arg("Hkv"),
        py::arg("S"));
  m.def("attn_decode_splits", &dmlamd::attn_decode_splits,
        "The split count attn_decode runs with (num_splits, or the automatic choice for 0)",
        py::arg("B"), py::arg("Hkv"), py::arg("Nmax"), py::arg("num_splits"), py::arg("device"));
  m.def("attn_decode_tiled", &dmlamd::attn_decode_tiled,
        "Tiled split-KV attention over a K/V cache for any R = (H/Hkv)*Nq >= 1 columns per K/V "
        "head: 16-column MFMA tiles, up to four per block (MFMA bf16, D=64 or 128 by q's last "
        "dim; num_splits 0 = auto). With an int32 block_table [B, max_pages] the caches are page "
        "pools [num_pages, Hkv, page_size, D], page_size % 32 == 0, and max_pages * page_size "
        "stands for Nmax",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_len"), py::arg("o"),
        py::arg("lse"), py::arg("ws"), py::arg("scale"), py::arg("causal"), py::arg("num_splits"),
        py::arg("block_table") = py::none());
  m.def("kvcache_append", &dmlamd::kvcache_append,
        "Write k_new / v_new [B, Hkv, Nq, D] into a dense [B, Hkv, Nmax, D] or, with a block_table, "
        "paged [num_pages, Hkv, page_size, D] K/V cache at the positions sdpa_kvcache gives the "
        "same rows (kv_len already counts them); one launch, no host sync",
        py::arg("k_new"), py::arg("v_new"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("kv_len"), py::arg("block_table") = py::none());
  m.def("attn_decode_tiled_workspace_floats", &dmlamd::attn_decode_tiled_workspace_floats,
        "fp32 elements attn_decode_tiled's workspace needs for R columns, S splits and head dim D",
        py::arg("B"), py::arg("Hkv"), py::arg("R"), py::arg("S"), py::arg("D") = 64);
  m.def("attn_decode_tiled_splits", &dmlamd::attn_decode_tiled_splits,
        "The split count attn_decode_tiled runs with (num_splits, or the automatic choice for 0)",
        py::arg("B"), py::arg("Hkv"), py::arg("R"), py::arg("Nmax"), py::arg("num_splits"),
        py::arg("device"));
  m.def("attn_decode_fp8", &dmlamd::attn_decode_fp8,
        "attn_decode_tiled over a float8_e4m3fn K/V cache (dense or paged, D=64 or 128, any R): the "
        "bytes are dequantised to bf16 in registers, key row j of K/V head h is "
        "float(cache[.., h, j, :]) * scale[h] with optional fp32 [Hkv] device tensors k_scale, "
        "v_scale (none = ones). Sized by attn_decode_tiled_splits / _workspace_floats",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_len"), py::arg("o"),
        py::arg("lse"), py::arg("ws"), py::arg("scale"), py::arg("causal"), py::arg("num_splits"),
        py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none(),
        py::arg("block_table") = py::none());
  m.def("kvcache_append_fp8", &dmlamd::kvcache_append_fp8,
        "kvcache_append into a float8_e4m3fn cache: element x is stored as "
        "e4m3_rne(clamp(float(x) / scale[h], -448, 448)); one launch, no host sync",
        py::arg("k_new"), py::arg("v_new"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("kv_len"), py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none(),
        py::arg("block_table") = py::none());
}
