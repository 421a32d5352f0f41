// Python bindings for the MI355X (gfx950) HIP kernels.
#include <torch/extension.h>

#include "ops.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "bert_pytorch_amd gfx950 HIP kernels";
  m.def("ln_fwd", &bpa::ln_fwd, "fused LayerNorm forward");
  // *_acc / acc: an existing gradient the result is added into in place;
  // that output then comes back as None
  m.def("ln_bwd", &bpa::ln_bwd, "fused LayerNorm backward", py::arg("dy"),
        py::arg("x"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("dgamma_acc") = py::none(), py::arg("dbeta_acc") = py::none());
  m.def("bias_gelu_fwd", &bpa::bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bpa::bias_gelu_bwd, py::arg("dy"), py::arg("x"),
        py::arg("bias"), py::arg("dbias_acc") = py::none());
  m.def("col_sum", &bpa::col_sum, "column sum [rows,H] -> fp32 [H]",
        py::arg("x"), py::arg("acc") = py::none(),
        py::arg("round_to") = py::none());
  m.def("gemm_bias_gelu_fwd", &bpa::gemm_bias_gelu_fwd,
        "hipblaslt GEMM with fused bias+GELU epilogue (+aux)");
  m.def("gemm_dgelu_bgrad", &bpa::gemm_dgelu_bgrad,
        "hipblaslt dgrad GEMM with fused dGELU+bias-grad epilogue");
  m.def("gemm_gelu_aux_supported", &bpa::gemm_gelu_aux_supported);
  m.def("bias_dropout_residual_ln_fwd", &bpa::bias_dropout_residual_ln_fwd);
  m.def("bias_dropout_residual_ln_bwd", &bpa::bias_dropout_residual_ln_bwd,
        py::arg("dy"), py::arg("z"), py::arg("mask"), py::arg("gamma"),
        py::arg("mean"), py::arg("rstd"), py::arg("p"), py::arg("has_bias"),
        py::arg("dy2") = py::none(), py::arg("dgamma_acc") = py::none(),
        py::arg("dbeta_acc") = py::none(), py::arg("dbias_acc") = py::none());
  m.def("embedding_ln_dropout_fwd", &bpa::embedding_ln_dropout_fwd);
  m.def("embedding_ln_dropout_bwd", &bpa::embedding_ln_dropout_bwd);
  m.def("ce_fwd", &bpa::ce_fwd);
  m.def("ce_bwd", &bpa::ce_bwd);
  m.def("attention_fwd", &bpa::attention_fwd);
  m.def("attention_bwd", &bpa::attention_bwd);
  m.def("attention_varlen_fwd", &bpa::attention_varlen_fwd,
        "packed [T_pad,3H] attention over a cu_seqlens index");
  m.def("attention_varlen_bwd", &bpa::attention_varlen_bwd);
  m.def("pack_rows", &bpa::pack_rows,
        "[B*S,H] -> [T_pad,H]: row i to row dest[i], dest<0 dropped");
  m.def("unpack_rows", &bpa::unpack_rows,
        "[T_pad,H] -> [B*S,H]: inverse of pack_rows, dropped rows zero");
  m.def("tr16_probe", &bpa::tr16_probe);
  m.def("wgrad_tn", &bpa::wgrad_tn, py::arg("dy"), py::arg("x"),
        py::arg("splitk_override") = 0, py::arg("acc") = py::none());
  m.def("wgrad_tn_supported", &bpa::wgrad_tn_supported);
  m.def("mlm_head_fwd", &bpa::mlm_head_fwd,
        "MFMA MLM-decoder GEMM with fused bias + CE-forward epilogue");
  m.def("mlm_head_eval", &bpa::mlm_head_eval,
        "mlm_head_fwd without the logits: loss/count/correct sums, lse, "
        "top-1 prediction");
  m.def("mlm_head_supported", &bpa::mlm_head_supported);
  m.def("wgrad_tn_profitable", &bpa::wgrad_tn_profitable);
  m.def("kfac_factor_update", &bpa::kfac_factor_update,
        "in-place K-FAC factor EMA: symmetric MFMA x^T x (+ bias column)",
        py::arg("x"), py::arg("factor"), py::arg("coef"),
        py::arg("has_bias"), py::arg("splitk_override") = 0);
  m.def("kfac_factor_supported", &bpa::kfac_factor_supported);
  m.def("mlm_mask", &bpa::mlm_mask,
        "dynamic MLM masking + padded-gather positions from raw shard rows",
        py::arg("input_ids"), py::arg("special"), py::arg("sample_index"),
        py::arg("count_table"), py::arg("seed"), py::arg("epoch"),
        py::arg("max_pred"), py::arg("vocab_size"), py::arg("mask_token"),
        py::arg("t_keep"), py::arg("t_rand"), py::arg("dense_labels") = false);
  m.def("mlm_mask_whole_word", &bpa::mlm_mask_whole_word,
        "mlm_mask with whole-word masking from a uint8 continuation table",
        py::arg("input_ids"), py::arg("special"), py::arg("sample_index"),
        py::arg("count_table"), py::arg("word_continues"), py::arg("seed"),
        py::arg("epoch"), py::arg("max_pred"), py::arg("vocab_size"),
        py::arg("mask_token"), py::arg("t_keep"), py::arg("t_rand"),
        py::arg("dense_labels") = false);
  m.def("mlm_mask_span", &bpa::mlm_mask_span,
        "mlm_mask with spans of whole words from a span-length table",
        py::arg("input_ids"), py::arg("special"), py::arg("sample_index"),
        py::arg("count_table"), py::arg("word_continues"),
        py::arg("span_table"), py::arg("seed"), py::arg("epoch"),
        py::arg("max_pred"), py::arg("vocab_size"), py::arg("mask_token"),
        py::arg("t_keep"), py::arg("t_rand"), py::arg("dense_labels") = false);
  m.def("multi_tensor_l2norm_sq", &bpa::multi_tensor_l2norm_sq);
  m.def("multi_tensor_clip_scale", &bpa::multi_tensor_clip_scale);
  m.def("fused_lamb", &bpa::fused_lamb);
  m.def("fused_adam", &bpa::fused_adam);
  m.def("tok_create_wordpiece", &bpa_tok::create_wordpiece);
  m.def("tok_encode_wordpiece", &bpa_tok::encode_wordpiece);
  m.def("tok_create_bpe", &bpa_tok::create_bpe);
  m.def("tok_encode_bpe", &bpa_tok::encode_bpe);
  m.def("tok_train_bpe", &bpa_tok::train_bpe);
}
