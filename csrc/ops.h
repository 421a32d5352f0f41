// Prototypes of every entry point bind.cpp binds and of the host helpers
// one .hip file calls in another. bind.cpp and each defining file include
// it, so a definition that drifts from its declaration fails to compile.
// With BPA_TOK_ONLY defined only the tokenizer core is declared and torch
// is not needed (the stand-alone sanitizer build of csrc/tok).
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace bpa_tok {
int64_t create_wordpiece(std::vector<std::string> vocab, std::string unk);
std::pair<std::vector<std::string>, std::vector<int64_t>> encode_wordpiece(
    int64_t handle, std::vector<std::string> words);
int64_t create_bpe(std::vector<std::string> vocab,
                   std::vector<std::string> merge_lines);
std::pair<std::vector<std::string>, std::vector<int64_t>> encode_bpe(
    int64_t handle, std::vector<std::string> pretokens);
std::vector<std::string> train_bpe(std::vector<std::string> words,
                                   std::vector<int64_t> counts,
                                   int64_t num_merges);
}  // namespace bpa_tok

#ifndef BPA_TOK_ONLY
#include <torch/extension.h>

namespace bpa {

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor gamma,
                                  torch::Tensor beta, double eps);
std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor x,
                                  torch::Tensor gamma, torch::Tensor mean,
                                  torch::Tensor rstd,
                                  c10::optional<torch::Tensor> dgamma_acc,
                                  c10::optional<torch::Tensor> dbeta_acc);
torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor bias);
std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor bias,
                                         c10::optional<torch::Tensor> dbias_acc);
// `acc` (fp32 [H]): acc += round_to(column sum), nothing is returned
torch::Tensor col_sum(
    torch::Tensor x, c10::optional<torch::Tensor> acc = c10::nullopt,
    c10::optional<torch::ScalarType> round_to = c10::nullopt);
// layernorm.hip, shared by the backward entry points: fold [nparts, S]
// fp32 partials over rows in a fixed order. `dsts` cuts the [S] result
// into dsts.size() equal segments; a segment with a destination (fp32) is
// added to it, after rounding through `round_to` if that is a 16-bit type,
// and its part of the returned tensor is then undefined.
torch::Tensor col_reduce_full(
    torch::Tensor parts,
    const std::vector<c10::optional<torch::Tensor>>& dsts = {},
    c10::optional<torch::ScalarType> round_to = c10::nullopt);
std::vector<torch::Tensor> gemm_bias_gelu_fwd(torch::Tensor x,
                                              torch::Tensor w1,
                                              torch::Tensor b1);
std::vector<torch::Tensor> gemm_dgelu_bgrad(torch::Tensor dout,
                                            torch::Tensor w2,
                                            torch::Tensor aux);
bool gemm_gelu_aux_supported();
std::vector<torch::Tensor> bias_dropout_residual_ln_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> bias, torch::Tensor residual,
    torch::Tensor gamma, torch::Tensor beta, double p, double eps,
    int64_t seed, int64_t offset);
std::vector<torch::Tensor> bias_dropout_residual_ln_bwd(
    torch::Tensor dy, torch::Tensor z, torch::Tensor mask, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd, double p, bool has_bias,
    c10::optional<torch::Tensor> dy2, c10::optional<torch::Tensor> dgamma_acc,
    c10::optional<torch::Tensor> dbeta_acc,
    c10::optional<torch::Tensor> dbias_acc);
std::vector<torch::Tensor> embedding_ln_dropout_fwd(
    torch::Tensor ids, c10::optional<torch::Tensor> tt, torch::Tensor word,
    torch::Tensor pos, c10::optional<torch::Tensor> tok, torch::Tensor gamma,
    torch::Tensor beta, double p, double eps, int64_t seed, int64_t offset,
    torch::ScalarType out_dtype);
std::vector<torch::Tensor> embedding_ln_dropout_bwd(
    torch::Tensor dy, torch::Tensor ids, c10::optional<torch::Tensor> tt,
    torch::Tensor z, torch::Tensor mask, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd, double p, int64_t vocab,
    int64_t max_pos, int64_t n_types);
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor labels,
                                  int64_t ignore_index);
torch::Tensor ce_bwd(torch::Tensor dloss, torch::Tensor logits,
                     torch::Tensor labels, torch::Tensor lse,
                     torch::Tensor count, int64_t ignore_index);
std::vector<torch::Tensor> attention_fwd(torch::Tensor qkv,
                                         torch::Tensor seqlens,
                                         int64_t num_heads, double p,
                                         int64_t seed, int64_t offset);
torch::Tensor tr16_probe(int64_t addr_mode);
// `acc` ([M, N], dy's dtype): acc += dW in place, nothing is returned
torch::Tensor wgrad_tn(torch::Tensor dy, torch::Tensor x,
                       int64_t splitk_override,
                       c10::optional<torch::Tensor> acc);
std::vector<torch::Tensor> mlm_head_fwd(torch::Tensor h, torch::Tensor w,
                                        torch::Tensor bias,
                                        torch::Tensor labels,
                                        int64_t ignore_index);
// logits-free evaluation instantiation of the same kernel:
// {loss_sum, count, correct, lse [P], pred [P] i32}
std::vector<torch::Tensor> mlm_head_eval(torch::Tensor h, torch::Tensor w,
                                         torch::Tensor bias,
                                         torch::Tensor labels,
                                         int64_t ignore_index);
bool mlm_head_supported(int64_t P, int64_t V, int64_t K);
bool wgrad_tn_supported(int64_t K, int64_t M, int64_t N);
bool wgrad_tn_profitable(int64_t K, int64_t M, int64_t N);
// kfac_factor.hip: factor[D,D] = coef[0]*factor + coef[1]*cov([x,1] or x),
// D = K + has_bias; coef = {beta, alpha} fp32 on the device
void kfac_factor_update(torch::Tensor x, torch::Tensor factor,
                        torch::Tensor coef, bool has_bias,
                        int64_t splitk_override);
bool kfac_factor_supported(int64_t N, int64_t K);
torch::Tensor attention_bwd(torch::Tensor dout, torch::Tensor qkv,
                            torch::Tensor seqlens, torch::Tensor out,
                            torch::Tensor lse, torch::Tensor dmask,
                            int64_t num_heads, double p, int64_t seed,
                            int64_t offset);
std::vector<torch::Tensor> attention_varlen_fwd(
    torch::Tensor qkv, torch::Tensor cu_seqlens, int64_t max_seqlen,
    int64_t num_heads, double p, int64_t seed, int64_t offset);
torch::Tensor attention_varlen_bwd(torch::Tensor dout, torch::Tensor qkv,
                                   torch::Tensor cu_seqlens,
                                   int64_t max_seqlen, torch::Tensor out,
                                   torch::Tensor lse, torch::Tensor dmask,
                                   int64_t num_heads, double p,
                                   int64_t seed, int64_t offset);
torch::Tensor pack_rows(torch::Tensor x, torch::Tensor dest, int64_t t_pad);
torch::Tensor unpack_rows(torch::Tensor y, torch::Tensor dest,
                          int64_t padded_rows);
// mlm_mask.hip: dynamic MLM masking of raw shard rows. input_ids i32 [B,S],
// special i32 [B,3], sample_index i64 [B], count_table i32 [S+1] ->
// {masked_ids, token_type_ids, attention_mask} i64 [B,S], {positions,
// gathered_labels} i64 [B*max_pred] (+ dense labels i64 [B,S] on request).
// seed carries the bits of a uint64; t_keep, t_rand are in units of 2^-32.
std::vector<torch::Tensor> mlm_mask(torch::Tensor input_ids,
                                    torch::Tensor special,
                                    torch::Tensor sample_index,
                                    torch::Tensor count_table, int64_t seed,
                                    int64_t epoch, int64_t max_pred,
                                    int64_t vocab_size, int64_t mask_token,
                                    int64_t t_keep, int64_t t_rand,
                                    bool dense_labels);
// The same with whole-word masking: word_continues u8 [vocab_size] is 1 where
// a vocabulary entry continues a word; words are masked whole or not at all.
std::vector<torch::Tensor> mlm_mask_whole_word(
    torch::Tensor input_ids, torch::Tensor special, torch::Tensor sample_index,
    torch::Tensor count_table, torch::Tensor word_continues, int64_t seed,
    int64_t epoch, int64_t max_pred, int64_t vocab_size, int64_t mask_token,
    int64_t t_keep, int64_t t_rand, bool dense_labels);
// The same with span masking: span_table i64 [Lmax <= 32] holds the clipped
// geometric law of the span length in units of 2^-32; a taken word grows over
// the words that follow it and the span shares one keep/random/mask decision.
std::vector<torch::Tensor> mlm_mask_span(
    torch::Tensor input_ids, torch::Tensor special, torch::Tensor sample_index,
    torch::Tensor count_table, torch::Tensor word_continues,
    torch::Tensor span_table, int64_t seed, int64_t epoch, int64_t max_pred,
    int64_t vocab_size, int64_t mask_token, int64_t t_keep, int64_t t_rand,
    bool dense_labels);
torch::Tensor multi_tensor_l2norm_sq(std::vector<torch::Tensor> tensors);
void multi_tensor_clip_scale(std::vector<torch::Tensor> grads,
                             torch::Tensor gnorm_sq, double max_norm);
void fused_lamb(std::vector<torch::Tensor> params,
                std::vector<torch::Tensor> grads,
                std::vector<torch::Tensor> ms, std::vector<torch::Tensor> vs,
                torch::Tensor gnorm_sq, double lr, double beta1, double beta2,
                double eps, double wd, int64_t step, bool bias_correction,
                bool grad_averaging, double max_grad_norm, bool use_ratio);
void fused_adam(std::vector<torch::Tensor> params,
                std::vector<torch::Tensor> grads,
                std::vector<torch::Tensor> ms, std::vector<torch::Tensor> vs,
                double lr, double beta1, double beta2, double eps, double wd,
                int64_t step, bool bias_correction, bool adam_w);

}  // namespace bpa

#endif  // BPA_TOK_ONLY
