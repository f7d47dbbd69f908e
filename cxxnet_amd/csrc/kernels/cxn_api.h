// The C ABI of libcxxnet_kernels.so: the one declaration of every exported cxn_* entry point and of
// the operand record they share.  Two readers depend on it:
//   * the compiler -- common.h includes this file, so a definition that disagrees with its prototype
//     in a count, a scalar width or a pointer type fails to compile ("conflicting types");
//   * cxxnet_amd/native.py -- derives the ctypes argtypes / restype of every entry point and the
//     fields of CxnOperand from this text, so the grammar is kept narrow:
//       - every prototype is  CXN_API <ret> cxn_name(<type> <name>, ...);  and may wrap over lines;
//       - every parameter is named, and no comment appears inside a parameter list;
//       - return types are int, long, void * and void;
//       - scalar parameters are int, long, float and uint32_t / unsigned; everything else is a pointer;
//       - the struct's members follow the same rules, one  <type> <name>;  each;
//       - between prototypes only // comments, # lines, the struct and its static_asserts appear.
//     native.py raises on anything else, and the build fails when the library's exported cxn_*
//     symbols and the names below differ (build.py _check_exports).
#pragma once
#include <stddef.h>

#define CXN_API extern "C" __attribute__((visibility("default")))

// One GEMM operand (cxn_gemm, cxn_gemm_glds*): a plain matrix (ptr, ld, rows, kdim, gstride per
// group) or, in the gather modes, the NHWC tensor and conv geometry the matrix is gathered from.
struct CxnOperand {
  const void *ptr;
  long gstride;
  long nbytes;
  int ld;
  int rows;
  int kdim;
  int H;
  int W;
  int C;
  int Ho;
  int Wo;
  int KH;
  int KW;
  int stride;
  int pad_h;
  int pad_w;
  int dil;
  int Cg;
};
static_assert(sizeof(CxnOperand) == 88, "CxnOperand layout is part of the ABI");
static_assert(offsetof(CxnOperand, ld) == 24, "CxnOperand layout is part of the ABI");
static_assert(offsetof(CxnOperand, Cg) == 80, "CxnOperand layout is part of the ABI");

// launch_list.hip
CXN_API int cxn_rec_begin();
CXN_API void *cxn_rec_end();
CXN_API int cxn_rec_size(void *list);
CXN_API int cxn_rec_replay(void *list, void *stream);
CXN_API int cxn_rec_replay_many(void *const *lists, int n, void *stream);
CXN_API void cxn_rec_free(void *list);
CXN_API int cxn_copy_d2d(void *dst, const void *src, long bytes, void *stream);
CXN_API int cxn_zero_ranges(float *base, const long *off, const long *len, int n, void *stream);
CXN_API int cxn_zero(void *dst, long bytes, void *stream);

// gemm_mfma.hip
CXN_API int cxn_gemm(const CxnOperand *a, const CxnOperand *b, int amode, int bmode, int va, int vb, void *out,
                     long out_gstride, int ldc, float alpha, const float *bias, long bias_gstride, int relu,
                     int mask_relu, int epi, int tile, int groups, int ksplit, long kstride, void *stream);

// gemm_glds.hip
CXN_API int cxn_gemm_set_group(int group_i);
CXN_API int cxn_gemm_glds(const CxnOperand *a, const CxnOperand *b, int amode, int bmode, void *out,
                          long out_gstride, int ldc, float alpha, const float *bias, long bias_gstride, int relu,
                          int mask_relu, int epi, int tile, int groups, int ksplit, long kstride, float *dbias,
                          float *dws, long dws_elems, int dws_ld, void *stream);
CXN_API int cxn_gemm_glds_add(const CxnOperand *a, const CxnOperand *b, int amode, int bmode, void *out,
                              long out_gstride, int ldc, const void *add, int mask_relu, int tile, int groups,
                              void *stream);
CXN_API int cxn_gemm_glds_split(const CxnOperand *a, const CxnOperand *b, int amode, int bmode, void *out, int ldc,
                                void *out2, int ldc2, int split_i, const float *bias, int relu, int tile,
                                void *stream);
CXN_API int cxn_gemm_set_sgd_stream(int mode);
CXN_API int cxn_gemm_set_sgd_stream_blocks(int blocks);
CXN_API long cxn_gemm_sgd_stream_calls();
CXN_API int cxn_gemm_glds_sgd(const CxnOperand *a, const CxnOperand *b, int ldc, float alpha, float *w, float *m,
                              void *wb, float lr, float wd, float mom, float clip, const float *hyp, int tile,
                              void *stream);

// conv_direct.hip
CXN_API long cxn_conv_direct(const void *x, int ldx, const void *w, const float *bias, void *y, int ldy, float *dbp,
                             long dbp_elems, float *db, int N, int H, int W, int Cg, int Cog, int groups, int KS,
                             int relu, int epi, int variant, void *stream);

// conv_wgrad_direct.hip
CXN_API long cxn_conv_wgrad_direct(const void *x, const void *dy, float *dw, float *db, float *ws, long ws_floats,
                                   int N, int H, int W, int C, int ldy, int Cg, int Cog, int groups, int KH, int KW,
                                   int pad_h, int pad_w, int stride, int splits, float alpha, void *stream);

// conv_rowrun.hip
CXN_API int cxn_conv_rowrun_fwd(const void *x, long x_bytes, const void *w, const float *bias, void *y, int N,
                                int H, int W, int C, int Ho, int Wo, int Cout, int KH, int LP, int S, int ldc,
                                int relu, void *stream);

// conv_rowrun_direct.hip
CXN_API long cxn_conv_wgrad_rowrun(const void *x, const void *dy, float *dw, float *ws, long ws_floats, int N,
                                   int H, int W, int C, int Ho, int Wo, int Cout, int ldy, int KH, int KW,
                                   int stride, int pad, float alpha, void *stream);
CXN_API int cxn_conv_rowrun_fwd2(const void *x, const void *w, const float *bias, void *y, int N, int H, int W,
                                 int C, int Ho, int Wo, int Cout, int ldc, int KH, int KW, int stride, int pad,
                                 int relu, void *stream);

// conv_fewc.hip
CXN_API int cxn_conv_fewc_fwd(const void *x, const void *w, const float *bias, void *y, int N, int H, int W, int Ho,
                              int Wo, int Cout, int KH, int KW, int S, int P, int ldc, int relu, void *stream);

// layout_kernels.hip
CXN_API int cxn_nchw_f32_to_nhwc_bf16(const float *x, void *y, int N, int C, int H, int W, int Cp, int Wp,
                                      float scale, void *stream);
CXN_API int cxn_image_u8_to_nhwc_bf16(const void *pix, const int *prm, const float *cm, const float *mean, int B,
                                      int h, int w, int C, int Cp, int Wp, int Hm, int Wm, int mode, float scale,
                                      void *y, void *stream);
CXN_API int cxn_nhwc_bf16_to_nchw_f32(const void *x, float *y, int N, int C, int H, int W, int Cp, int Wp,
                                      void *stream);
CXN_API int cxn_transpose(const void *x, void *y, int B, int R, int Cc, void *stream);
CXN_API int cxn_conv_weight_flip(const void *w, void *wt, int G, int Co, int KH, int KW, int Ci, void *stream);
CXN_API int cxn_conv_weight_flip_multi(const void *const *ws, void *const *wts, const int *dims, int n, void *stream);

// pool_kernels.hip
CXN_API int cxn_pool_fwd(const void *x, void *y, void *arg, int N, int H, int W, int C, int Ho, int Wo, int KH,
                         int KW, int S, int P, int mode, int relu, void *stream);
CXN_API int cxn_pool_bwd_tie_all(const void *x, const void *y, const void *dy, void *dx, int N, int H, int W, int C,
                                 int Ho, int Wo, int KH, int KW, int S, int P, int relu, void *stream);
CXN_API int cxn_pool_bwd(const void *x, const void *arg, const void *dy, void *dx, int N, int H, int W, int C,
                         int Ho, int Wo, int KH, int KW, int S, int P, int mode, int relu, float *db, float *ws,
                         long ws_elems, void *stream);

// lrn_kernels.hip
CXN_API int cxn_lrn_fwd(const void *x, void *y, long npix, int C, int nsize, float alpha, float beta, float knorm,
                        void *stream);
CXN_API int cxn_pool_lrn_fwd(const void *x, void *P, void *arg, void *Y, int N, int Hin, int Win, int C, int Ho,
                             int Wo, int relu, int nsize, float alpha, float beta, float knorm, void *stream);
CXN_API int cxn_lrn_pool_bwd(const void *P, const void *dY, const void *arg, void *dx, int N, int Hin, int Win,
                             int C, int Ho, int Wo, int relu_bit, int nsize, float alpha, float beta, float knorm,
                             float *dbias, float *dbias_part, long part_rows, int det, void *stream);
CXN_API int cxn_lrn_bwd_db(const void *x, const void *dy, void *dx, long npix, int C, int nsize, float alpha,
                           float beta, float knorm, int mask_relu, float *db, float *part, long part_floats,
                           void *stream);
CXN_API int cxn_lrn_bwd(const void *x, const void *dy, void *dx, long npix, int C, int nsize, float alpha,
                        float beta, float knorm, int mask_relu, void *stream);

// act_kernels.hip
CXN_API int cxn_act_fwd(const void *x, void *y, void *y2, long n, int kind, float b, void *stream);
CXN_API int cxn_act_bwd(const void *y, const void *dy, void *dx, long n, int kind, float b, void *stream);
CXN_API int cxn_dropout(const void *x, void *y, long n, unsigned seed, const int *counter, float pkeep, void *stream);

// loss_kernels.hip
CXN_API int cxn_metric_eval(const float *p, int ldp, const float *lab, int ldl, int lw, int B, int K, int nm,
                            const int *kinds, const int *args, double *acc, float *part, void *stream);
CXN_API int cxn_softmax(const void *x, void *y, float *pf, int rows, int K, void *stream);
CXN_API int cxn_loss_grad(const float *p32, void *node, const float *label, int rows, int K, int lw, float scale,
                          int kind, void *stream);

// reduce_kernels.hip
CXN_API int cxn_colsum(const void *dy, float *db, long rows, int C, float *ws, long ws_elems, void *stream);
CXN_API int cxn_colsum_multi(const void *const *dys, float *const *dbs, const long *rows, const int *Cs,
                             const void *const *masks, int n, void *stream, const long *lds);
CXN_API int cxn_set_deterministic(int on);
CXN_API int cxn_set_kernel_variant(int which, int v);
CXN_API int cxn_splitk_accumulate(const float *ws, int nsplit, long slab, float *out, void *stream);
CXN_API int cxn_splitk_finalize(const float *ws, int nsplit, long slab, void *out, long rows, int cols,
                                const float *bias, int relu, int mask_relu, void *stream);
CXN_API int cxn_splitk_finalize_dropout(const float *ws, int nsplit, long slab, void *out, long rows, int cols,
                                        const float *bias, int relu, unsigned seed, const int *counter, float pkeep,
                                        void *stream);

// copy_kernels.hip
CXN_API int cxn_cast_f32_bf16(const float *x, void *y, long n, void *stream);
CXN_API int cxn_add_bf16(const void *a, const void *b, void *y, long n, void *stream);
CXN_API int cxn_fanout_bf16(const void *src, void *d0, void *d1, void *d2, void *d3, int nd, long n, void *stream);
CXN_API int cxn_sum_bf16(const void *s0, const void *s1, const void *s2, const void *s3, int ns, void *y, long n,
                         void *stream, int mask);
CXN_API int cxn_concat(void *const *ins, const int *cs, int n, void *out, int Ct, long npix, int bwd, int mask,
                       void *stream);
CXN_API int cxn_channel_copy(const void *src, int Cs, int soff, void *dst, int Cd, int doff, int Cc, long npix,
                             int accumulate, void *stream);
CXN_API int cxn_pad_interior(const void *src, void *dst, int N, int H, int W, int C, int H2, int W2, int py, int px,
                             void *stream);
CXN_API int cxn_add_rows_f32(const float *src, float *dst, long rows, int L, int Ls, void *stream);
CXN_API int cxn_pad_rows(const void *src, void *dst, long rows, int L, int Lp, void *stream);

// layer_kernels.hip
CXN_API int cxn_rand_fill(float *out, long n, unsigned seed, int dist, float a, float b, void *stream);
CXN_API int cxn_chan_reduce(const void *x, const void *g, const float *mean, float *out, long rows, int C, int mode,
                            void *stream);
CXN_API int cxn_bn_stats(const void *x, float *stats, float *mean, float *inv, long rows, int C, float eps,
                         void *stream);
CXN_API int cxn_bn_fwd(const void *x, void *y, void *xhat, void *xsave, const float *mean, const float *inv,
                       const float *slope, const float *bias, long rows, int C, void *stream);
CXN_API int cxn_bn_bwd(const void *g, const void *xsave, void *dx, const float *mean, const float *inv,
                       const float *slope, float *gslope, float *gbias, float *sums, float *coef, long rows, int C,
                       void *stream);
CXN_API int cxn_prelu(const void *x, const void *g, void *y, const float *slope, long rows, int C, unsigned seed,
                      const int *counter, float rnd, int mode, void *stream);
CXN_API int cxn_insanity(const void *x, const void *g, void *y, void *y2, long n, float lb, float ub, int train,
                         unsigned seed, const int *counter, int mode, void *stream);
CXN_API int cxn_ins_pool_fwd(const void *x, void *y, void *ysave, int N, int H, int W, int C, int Ho, int Wo, int K,
                             int S, float keep, unsigned seed, const int *counter, void *stream);
CXN_API int cxn_ins_pool_bwd(const void *x, const void *ypool, const void *gy, void *dx, int N, int H, int W, int C,
                             int Ho, int Wo, int K, int S, float keep, unsigned seed, const int *counter,
                             void *stream);

// bn_ma_kernels.hip
CXN_API long cxn_bn_ma_ws_floats(long rows, int C);
CXN_API int cxn_bn_ma_fwd_train(const void *x, void *y, void *xsave, const float *slope, const float *bias,
                                float *stat, float *rmean, float *rvar, float *ws, long ws_floats, long rows, int C,
                                float eps, float mom, void *stream);
CXN_API int cxn_bn_ma_fwd_infer(const void *x, void *y, const float *slope, const float *bias, const float *rmean,
                                const float *rvar, float *stat, long rows, int C, float eps, void *stream);
CXN_API int cxn_bn_ma_bwd(const void *g, const void *x, void *dx, const float *slope, float *gslope, float *gbias,
                          const float *stat, float *coef, float *ws, long ws_floats, long rows, int C, void *stream);

// gn_kernels.hip
CXN_API long cxn_gn_ws_floats(long B, long HW, int C);
CXN_API int cxn_gn_fwd(const void *x, void *y, const float *slope, const float *bias, float *mean, float *rstd,
                       float *ws, long ws_floats, long B, long HW, int C, int groups, float eps, void *stream);
CXN_API int cxn_gn_bwd(const void *g, const void *x, void *dx, const float *slope, float *gslope, float *gbias,
                       const float *mean, const float *rstd, float *coef, float *ws, long ws_floats, long B, long HW,
                       int C, int groups, void *stream);

// add_kernels.hip
CXN_API int cxn_add_fwd(const void *x0, const void *x1, const void *x2, const void *x3, int n_in, void *y,
                        void *mask, long n, int relu, void *stream);
CXN_API int cxn_add_bwd(const void *g, const void *mask, void *d0, void *d1, void *d2, void *d3, int n_out, long n,
                        void *stream);

// hact_kernels.hip
CXN_API long cxn_hact_pass_elems();
CXN_API int cxn_hact_fwd(const void *x, void *y, long n, int kind, void *stream);
CXN_API int cxn_hact_bwd(const void *x, const void *g, void *dx, long n, int kind, void *stream);

// silu_kernels.hip
CXN_API long cxn_silu_pass_elems();
CXN_API int cxn_silu_fwd(const void *x, void *y, long n, void *stream);
CXN_API int cxn_silu_bwd(const void *x, const void *g, void *dx, long n, void *stream);

// droppath_kernels.hip
CXN_API long cxn_drop_path_pass_elems();
CXN_API int cxn_drop_path(void *x, long B, long n, unsigned seed, const int *counter, float pkeep, void *stream);

// se_kernels.hip
CXN_API int cxn_se_parts(long B, long HW, int C);
CXN_API long cxn_se_ws_floats(long Bmax, long HW, int C);
CXN_API int cxn_ch_scale_fwd(const void *x, const void *s, void *y, long B, long HW, int C, void *stream);
CXN_API int cxn_ch_scale_bwd(const void *g_, const void *x, const void *s, void *dx, void *ds, float *ws,
                             long ws_floats, long B, long HW, int C, void *stream);
CXN_API int cxn_global_pool_fwd(const void *x, void *y, float *ws, long ws_floats, long B, long HW, int C,
                                float scale, void *stream);

// dwconv_kernels.hip
CXN_API int cxn_dwconv_fwd(const void *x, long xs, const void *w, const float *bias, void *y, long ys, int N, int H,
                           int W, int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                           int relu, void *stream);
CXN_API int cxn_dwconv_bwd_data(const void *dy, long dys, const void *w, void *dx, long dxs, int N, int H, int W,
                                int C, int Cout, int groups, int KH, int KW, int stride, int pad_y, int pad_x,
                                int mask_relu, void *stream);
CXN_API int cxn_dwconv_bwd_weight(const void *x, long xs, const void *dy, long dys, float *dw, float *db, float *ws,
                                  long ws_floats, int N, int H, int W, int C, int Cout, int groups, int KH, int KW,
                                  int stride, int pad_y, int pad_x, void *stream);

// optim_kernels.hip
CXN_API int cxn_fused_update(const long *offs, const long *ns, const float *hyper, int nseg, float *w, float *g,
                             float *st1, float *st2, void *wb, int algo, float d1, float d2, void *stream);
CXN_API int cxn_nonfinite_check(const float *g, long n, int *flag, void *stream);
CXN_API int cxn_scale_f32(float *x, long n, float sc, void *stream);
CXN_API int cxn_add_i32(int *p, int v, void *stream);

// jpeg_kernels.hip
CXN_API int cxn_jpeg_idct(const void *coef, const int *bwin, const int *meta, long nblk, void *plane, void *stream);
CXN_API int cxn_jpeg_color(const void *plane, const int *meta, const int *prm, int B, int h, int w, int C,
                           void *out, void *stream);

// warp_kernels.hip
CXN_API int cxn_image_warp(const void *src, const void *table, const void *wtab, int r0, int r1, int h, int w,
                           int C, void *out, void *stream);
