// The one declaration of every host function that one .hip file defines and another calls (common.h includes this at its end, so every
// translation unit sees it, the defining one included: a definition that disagrees does not compile, a declaration without a definition
// does not link).  Default arguments live here only.  A function that only its own file calls is static there and is not listed.
#pragma once

// api.hip
// Raise a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) -- at most once per (device, kernel, size): the host call
// costs tens of microseconds, a dozen of them per step put the enqueue thread behind the GPU on slower hosts.  (A cache of what was
// already asked of the runtime, not dispatch state: the same launches happen with or without it.)
hipError_t mlsp_lds_limit(const void* fn, size_t lds);

// gemm.hip
// cx: the calling entry point's context (callctx.h: product mode, f16x3 operand bounds); no default, a call without one does not compile.
// The shape queries answer for cx's mode; the launchers also measure into / look up cx's operand bounds.
// unfold_dw / unfolded (nullable): common.h GemmOpts
int launch_slab_reduce(hipStream_t st, const float* slab, float* C, int M, int N, int ldc, int nsplit, float* unfold_dw = nullptr,
                       bool* unfolded = nullptr);
int gemm_stat_parts(const CallCtx& cx, int M, int N, int K);
int gemm_panel_rows(const CallCtx& cx, int M, int N, int K);
size_t gemm_slab_floats(int M, int N, int K);   // (the same in every mode)
int prof_cls_begin(hipStream_t st, int cls);   // cls: common.h MLSP_PROF_*; -> token (< 0: not armed)
void prof_cls_end(hipStream_t st, int token, double work);
// which: the operand that takes the transform, 1 = A ([M][K] row-major), 2 = B ([K][N] k-major) (common.h GemmXf)
bool gemm_xf_supported(const CallCtx& cx, bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, int which);
int gemm_bs_parts(const CallCtx& cx, int M, int N, int K, int lda, int ldb, int ldc);
bool gemm_dy_supported(const CallCtx& cx, bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb);
bool gemm_xf_on_split(const CallCtx& cx, bool ta, bool tb, int M, int N, int K, int which);
int launch_gemm(hipStream_t st, CallCtx& cx, bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                int ldc, const GemmOpts& o = GemmOpts());
int launch_gemm_mx(hipStream_t st, CallCtx& cx, bool ta, bool tb, int M, int N, int K, const void* A, int a_bf16, int lda, const void* B, int b_bf16,
                   int ldb, void* C, int c_bf16, int ldc, const GemmOpts& o = GemmOpts());

// knn.hip (the search kernels v1 - v5 and the launcher that follows knn_plan.h)
// xx_ws: [B*N] floats of workspace; planes (nullable): plane_bytes bytes of workspace for the v6 families (what the plan's plane_bytes asks)
int launch_knn(hipStream_t st, const float* x, int ld, int B, int N, int C, int k, int* idx, float* xx_ws, void* planes, size_t plane_bytes);
// the shapes knn6.hip's kernels take, as statements over knn_plan.h: vector-exact mode / knn6_kernel / knn6w_kernel
bool knn6_vex_supported(int B, int N, int C, int k);
bool knn6_supported(int B, int N, int C, int k);
bool knn6w_supported(int B, int N, int C, int k);

// knn6.hip (the v6 search kernels)
// p: the plan of the call (family VEX, V6 or V6W_V5); xx [B*N] floats and planes (the plan's plane_bytes) are workspace that the launch
// writes; *flags_out (V6W_V5): the per-cloud flags ([B] ints inside `planes`) the caller hands to the v5 launch behind it
struct KnnPlan;
int launch_knn6(hipStream_t st, const KnnPlan& p, const float* x, int ld, int B, int N, int C, int k, int* idx, float* xx, void* planes,
                int** flags_out);

// reverse.hip (the reverse neighbour index: not a search kernel)
int launch_group_reverse(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_ent);
int launch_group_reverse_compact(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_cnt, int* rev_ent, int* pad_cnt);
int launch_knn_reverse(hipStream_t st, const int* idx, int B, int N, int k, int* rev_off, int* rev_ent);

// bn.hip
int bn_vec_parts(int M);
int bn_stat_parts(int M);
int bn_parts_max(int M);
int launch_colstats_n(hipStream_t st, const float* Y, int M, int C, int ld, double* part, int* nparts_out);
int launch_colstats(hipStream_t st, const float* Y, int M, int C, int ld, double* part);
// bound_out (nullable, [C]): also write the channels' output bounds |gamma| sqrt(count) + |beta| (an entry that CallCtx::offered_output found)
int launch_bn_finalize(hipStream_t st, const double* part, int nparts, double count, int C, const float* gamma, const float* beta, float* run_mean,
                       float* run_var, float momentum, float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                       float* bound_out = nullptr);
int launch_bn_finalize_groups(hipStream_t st, const double* part, int nparts, double count, int C, const float* gamma, const float* beta,
                              float* run_mean, float* run_var, float momentum, float eps, float* scale, float* shift, float* save_mean,
                              float* save_invstd, float* gsum, int ppg);
int launch_bn_eval_prepare(hipStream_t st, int C, const float* gamma, const float* beta, const float* run_mean, const float* run_var, float eps,
                           float* scale, float* shift, float* save_mean, float* save_invstd);
int launch_bn_act_fwd(hipStream_t st, const float* Y, float* Z, size_t rows, int C, const float* scale, const float* shift, int act, float slope,
                      float p_drop, uint64_t seed);
// zero_vec (nullable, [C]; also launch_bn_act_bwd_b16, launch_skinny_bn_bwd_z and the *_z finalizers): the gradient of a bias in front of a
// batch-statistics BatchNorm, zero-filled by the pass's finalizer -- every MLSP_OK return has written it
int launch_bn_act_bwd(hipStream_t st, const float* dZ, const float* Y, float* dY, int M, int C, const float* scale, const float* shift,
                      const float* mean, const float* invstd, int training, int act, float slope, float p_drop, uint64_t seed, double* part,
                      float* dgamma, float* dbeta, float* mean_dz, float* mean_dzy, float* zero_vec, float* gpart = nullptr,
                      int rows_per_group = 0, int* gpart_slabs = nullptr, const double* pre_stats = nullptr, int pre_parts = 0);
int launch_bn_bwd_finalize_coef_z(hipStream_t st, const double* part, int nparts, double count, int C, const float* bn_save, float* dgamma,
                                  float* dbeta, float* coef, float* zero_vec);
int launch_bn_bwd_finalize_coef_groups(hipStream_t st, const double* part, int nparts, double count, int C, const float* bn_save, float* dgamma,
                                       float* dbeta, float* coef, const float* gys, int ppg, int rows, float* gout);
int launch_bn_bwd_finalize_z(hipStream_t st, const double* part, int nparts, double count, int C, float* dgamma, float* dbeta, float* mean_dz,
                             float* mean_dzy, float* zero_vec);
int launch_bn_bwd_finalize(hipStream_t st, const double* part, int nparts, double count, int C, float* dgamma, float* dbeta, float* mean_dz,
                           float* mean_dzy);
int launch_colsum_groups(hipStream_t st, const float* X, int G, int rows_per_group, int C, float* out, float* scratch = nullptr);
int launch_bn_dy_gbias(hipStream_t st, const float* Y, int G, int rows_per_group, int C, const double* stats, int panel_rows, const float* coef,
                       float* scratch, float* out, const float* ysum);
int launch_colsum_groups_fin(hipStream_t st, const float* scratch, int G, int C, int slabs, float* out);
int launch_colsum(hipStream_t st, const float* X, int M, int C, double* part, float* out);
int launch_bn_act_bwd_partials_vec(hipStream_t st, const float* dZ, const float* Y, int M, int C, const float* scale, const float* shift,
                                   const float* mean, const float* invstd, int act, float slope, double* part);
int launch_colmax_fwd(hipStream_t st, const float* Z, int B, int N, int C, float* out, int* arg);
int launch_colmax_bwd(hipStream_t st, const float* dOut, const int* arg, int B, int N, int C, float* dZ);
int launch_segmax_fwd(hipStream_t st, const float* Z, int P, int k, int C, float* out, uint8_t* argk);
int launch_segsel_act_fwd(hipStream_t st, const float* Y, int G, int k, int C, const float* scale, const float* shift, int act, float slope,
                          float* out, float* ysel, uint8_t* argk);
int launch_segsel_bwd_apply(hipStream_t st, const float* dOut, const float* Y, const float* ysel, const uint8_t* argk, size_t M, int k, int C,
                            const float* bn, const float* m1, const float* m2, int act, float slope, float* dY);
int launch_segmax_bwd(hipStream_t st, const float* dOut, const uint8_t* argk, int P, int k, int C, float* dZ);
int launch_bn_act_fwd_b16(hipStream_t st, const void* Y, void* Z, int rows, int C, const float* scale, const float* shift, int act, float slope,
                          float p_drop, uint64_t seed);
int launch_bn_act_bwd_b16(hipStream_t st, const void* dZ, const void* Y, void* dY, int M, int C, const float* scale, const float* shift,
                          const float* mean, const float* invstd, int training, int act, float slope, float p_drop, uint64_t seed, double* part,
                          float* dgamma, float* dbeta, float* mean_dz, float* mean_dzy, float* zero_vec);
int launch_colsum_groups_b16(hipStream_t st, const void* X, int G, int rows_per_group, int C, float* out, float* scratch);

// edge.hip
int edge_bwd_reduce_parts(int P, int Cout, const void* a, const void* b, const void* c, const void* d, const void* e, int lddo, int ldo);
int edge_reduce_parts(int P);
bool build_wd_leaves_bound(int Cout, int C);
int launch_build_wd(hipStream_t st, const float* W, int Cout, int C, float* Wd, float* amax = nullptr);
int launch_build_wd_eval(hipStream_t st, const float* W, int Cout, int C, float* Wd, int Ca, const float* ga, const float* ba, const float* rma,
                         const float* rva, float* sva, int Cb, const float* gb, const float* bb, const float* rmb, const float* rvb, float* svb,
                         float eps);
int launch_unbuild_wd(hipStream_t st, const float* dWd, int Cout, int C, float* dW);
int launch_edge_reduce(hipStream_t st, const float* uv, const int* idx, const float* gamma, int P, int N, int Cout, int k, float* ysel,
                       uint8_t* argsel, float* s1, double* part, int* nparts_used);
int launch_edge_select_act(hipStream_t st, const float* ysel, int P, int Cout, const float* scale, const float* shift, int act, float slope,
                           float* out, int ldo);
bool edge_bwd_leaves_duv_bound(const float* dOut, const float* out, const float* ysel, const float* uv, const float* s1, const uint8_t* argsel,
                               int Cout, const float* scale, const float* mean, const float* invstd, const float* gz, const float* duv, int lddo,
                               int ldo);
int launch_edge_bwd_reduce(hipStream_t st, const float* dOut, const float* out, const float* ysel, int P, int Cout, const float* scale,
                           const float* mean, const float* invstd, int act, float slope, double* part, int lddo, int ldo, float* gz,
                           float* duv_amax);
int launch_edge_bwd_point(hipStream_t st, const float* dOut, const float* out, const float* uv, const float* s1, int P, int Cout, int k,
                          const float* scale, const float* mean, const float* invstd, const float* mean_dz, const float* mean_dzy, int act,
                          float slope, float* gz, float* duv, int lddo, int ldo, float* duv_amax);
int launch_edge_bwd_gather(hipStream_t st, const float* gz, const uint8_t* argsel, const float* uv, const float* s1, int k, const int* rev_off,
                           const int* rev_ent, int P, int N, int Cout, const float* scale, const float* mean, const float* invstd,
                           const float* mean_dz, const float* mean_dzy, float* duv, float* duv_amax);
int launch_graph_feature_fwd(hipStream_t st, const float* x, const int* idx, int P, int N, int C, int k, float* F);
int launch_graph_feature_bwd(hipStream_t st, const float* dF, const int* rev_off, const int* rev_ent, int P, int N, int C, int k, float* dx);

// loss.hip
int launch_chamfer_fwd(hipStream_t st, const float* pred, const float* gold, const float* mask, int B, int N, float scale, float* per_cloud,
                       int* argA, int* argB, float* loss);
int launch_chamfer_bwd(hipStream_t st, const float* pred, const float* gold, const float* mask, int B, int N, float scale, const float* per_cloud,
                       const int* argA, const int* argB, const float* gout, float* dpred);
int launch_chamfer_dir_fwd(hipStream_t st, const float* p1, const float* p2, const float* mc, int B, int N, float* per_cloud, int* arg, float* loss);
int launch_chamfer_dir_bwd(hipStream_t st, const float* p1, const float* p2, const float* mc, int B, int N, const float* per_cloud, const int* arg,
                           const float* gout, float* dp1, float* dp2);
int launch_normal_loss_fwd(hipStream_t st, const float* pred, const float* gt, const float* w, int P, float weight, double* part, float* out);
int launch_normal_loss_bwd(hipStream_t st, const float* pred, const float* gt, const float* w, int P, float weight, const float* fwd_out,
                           const float* gout, float* dpred);
int launch_density_tail_fwd(hipStream_t st, const float* logits, const float* w, int P, int nc, float* pvec, float* dens);
int launch_density_tail_bwd(hipStream_t st, const float* pvec, const float* w, const float* dp, const float* dd, int P, int nc, float* dlogits);
int launch_density_loss_fwd(hipStream_t st, const float* pvec, const float* dens, const float* tvec, const float* target, const float* m, int P,
                            int nc, float dweight, double* part, float* out);
int launch_density_loss_bwd(hipStream_t st, const float* pvec, const float* dens, const float* tvec, const float* target, const float* m, int P,
                            int nc, float dweight, const float* fwd_out, const float* gkl, const float* gmae, float* dp, float* dd);

// tnet.hip
int tnet_grid(int ntiles);
int tnet_points_per_tile(int k);
int tnet_fwd_parts(int B, int N, int k);
int launch_tnet_edge_fwd(hipStream_t st, int mode, const float* uv, const int* idx, const float* bn1, const float* W2, const float* gamma2, int P, int N, int k,
                         float slope, float* zsel, uint8_t* argsel, double* part);
int launch_tnet_out(hipStream_t st, const float* zsel, const float* bn2, int P, float slope, float* out);
int launch_tnet_bwd_reduce(hipStream_t st, const float* dT, const float* T, const float* zsel, const float* bn2, int P, float slope, double* part);
int launch_tnet_bwd_g(hipStream_t st, const float* dT, const float* T, const float* bn2, const float* mean_dz, const float* mean_dzy, int P,
                      float slope, float* g, float* coef);
size_t tnet_bwd_scratch_floats(int ntiles);
int launch_tnet_edge_bwd(hipStream_t st, int mode, const float* uv, const int* idx, const float* bn1, const float* W2, const float* bn2, const float* g,
                         const uint8_t* argsel, const float* coef, int P, int N, int k, float slope, float* dhp, float* scratch, double* part1,
                         float* dW2, int* nparts);
int launch_tnet_edge_bwd2(hipStream_t st, const float* dhp, const float* uv, const float* s1, const float* bn1, const float* m1, const float* m2,
                          const int* rev_off, const int* rev_ent, int P, int N, int k, float* duv);
size_t tnet_w1_moment_doubles(int P, int k);
int launch_tnet_bwd_w1_moments(hipStream_t st, const float* dhp, const int* idx, const int* rev_off, const float* x, int ldx, const float* W1,
                               const float* bn1, const float* m1, const float* m2, int P, int N, int k, int C, double* scratch, float* dW1);

// colmax.hip
int launch_colsel(hipStream_t st, const float* Y, const float* gamma, int B, int N, int C, float* ysel, int* arg);
int launch_colsel_panels(hipStream_t st, const float* pv, const int* pr, const float* gamma, int B, int N, int C, int panel_rows, float* ysel,
                         int* arg, const float* bn, int act, float slope, float* out);
int launch_colsel_out(hipStream_t st, const float* ysel, const float* bn, int B, int C, int act, float slope, float* out);
int launch_colmax_bwd_coef(hipStream_t st, const float* dOut, const float* out, const float* ysel, const float* bn, int B, int C, double count,
                           int act, float slope, int training, float* g, float* coef, float* dgamma, float* dbeta);
int launch_wt_vec_neg_scale_rows(hipStream_t st, const float* W, int ldw, const float* v, const float* rowscale, int Cout, int Cin, float* negr,
                                 float* Wb);
int launch_colmax_gather_rows(hipStream_t st, const float* g, const int* arg, const float* X, int ldx, int B, int N, int Cout, int Cin, float* S);
int launch_colmax_dw(hipStream_t st, const float* S, const float* WG, const float* sx, const float* coef, const float* bn, int Cout, int Cin,
                     float* dW);
int launch_colmax_scatter_rows(hipStream_t st, const float* g, const int* arg, const float* W, int ldw, int B, int N, int Cout, int Cin, float* dX,
                               int lddx);

// labels.hip
int launch_radius_count(hipStream_t st, const float* x, int ld, int B, int N, float radius, int max_nn, int* count);
int launch_knn_normals(hipStream_t st, const float* x, int ld, const int* idx, int B, int N, int k, float* normals);

// skinny.hip
int launch_skinny_bwd_pair(hipStream_t st, const float* G, int ldg, const float* W, int ldw, const float* X, int ldx, float* dX, int lddx, float* dW,
                           int M, int Cin, int Cout, int dx_accumulate = 0);
int launch_skinny_gemm(hipStream_t st, bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                       const float* bias);
int launch_skinny_linear_bn_act(hipStream_t st, const float* X, int ldx, int M, int Cin, const float* W, int ldw, int Cout, const float* bias,
                                const float* gamma, const float* beta, float* run_mean, float* run_var, float momentum, float eps, int training,
                                int act, float slope, float p_drop, uint64_t seed, float* Y, float* Z, float* bn_save);
int launch_skinny_bn_bwd_z(hipStream_t st, const float* dZ, const float* Y, float* dY, int M, int C, const float* bn_save, int training, int act,
                           float slope, float p_drop, uint64_t seed, float* dgamma, float* dbeta, float* zero_vec);
int launch_compose_fwd(hipStream_t st, const float* Wa, const float* ba, const float* Wb, const float* bb, int Cm, int Ci, int Co, float* W,
                       float* b);
int launch_compose_bwd(hipStream_t st, const float* dW, const float* db, const float* Wa, const float* ba, const float* Wb, int Cm, int Ci, int Co,
                       float* dWa, float* dba, float* dWb);

// sa.hip
int launch_fps(hipStream_t st, const float* xyz, int ldx, int B, int N, int S, const int* start, int* out);
int launch_ball_query(hipStream_t st, const float* xyz, int ldx, const float* q, int ldq, int B, int N, int S, float r2, int nsample, int* idx);
int launch_sa_group_fwd(hipStream_t st, const float* xyz, int ldx, const float* feat, int D, const float* q, int ldq, const int* idx, int B, int N,
                        int S, int ns, float* G);
int launch_sa_group_bwd(hipStream_t st, const float* dG, int ldg, int col, int D, const int* rev_off, const int* rev_ent, int B, int N, int S, int ns,
                        float* dfeat);
int launch_knn_query(hipStream_t st, const float* ref, int ldr, int Nr, const float* qry, int ldq, int Nq, int B, int C, int k, int* idx,
                     float* dist);
int launch_interp3_fwd(hipStream_t st, const float* feat, const int* idx, const float* dist, int B, int N, int S, int D, float* out);
int launch_interp3_bwd(hipStream_t st, const float* dout, const float* dist, const int* rev_off, const int* rev_ent, int B, int N, int S, int D,
                       float* dfeat);
int sa_fold_parts(long E);
int launch_sa_fold_fwd(hipStream_t st, const float* u, const float* w, const int* idx, int B, int N, int S, int ns, int C, const float* gamma,
                       const float* beta, float* run_mean, float* run_var, float momentum, float eps, int training, float* Z, float* bn_save,
                       double* part);
int launch_sa_fold_bwd(hipStream_t st, const float* dZ, const float* u, const float* w, const int* idx, const int* rev_off, const int* rev_ent, int B,
                       int N, int S, int ns, int C, const float* bn_save, int training, float* du, float* dw, float* dgamma, float* dbeta,
                       double* part, float* mean_dz, float* mean_dzy, const int* rev_cnt, const int* pad_cnt);

// corrupt.hip
int launch_collapse_to_point(hipStream_t st, float* X, int B, int N, const int* choice, const float* u, const float* noise, float r2, int min_pts,
                             float* mask, int* chosen);
int launch_scan_select(hipStream_t st, const float* X, int B, int N, int C, const double* R, int pixel, float* Xs, float* mask);
int launch_region_assign(hipStream_t st, const float* X, int B, int C, int N, const float* thr, int n, float clip, int* Y);
int launch_deform_regions(hipStream_t st, float* X, int B, int C, int N, const int* regions, const int* order, int nreg, const float* lookup,
                          const float* noise, int min_pts, int groups, float* mask);
int launch_transform3_fwd(hipStream_t st, const float* x, const float* T, int B, int N, float* out);
int launch_transform3_bwd(hipStream_t st, const float* x, const float* T, const float* dout, int B, int N, float* dx, float* dT);

// thin.hip
size_t thin_tn_slab_floats(int M, int N, int K);
int thin_bs_parts(int M, int N, int K);
// reads o.bias, slab, slab_floats, xf, bs, unfold_dw, unfolded; launch_gemm keeps a launch with any other field set away from it
int launch_thin_gemm(hipStream_t st, bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                     const GemmOpts& o);
bool thin_xf_supported(bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, int which);

// multi.hip
int launch_xf_materialize(hipStream_t st, const float* X, int ldx, int M, int C, const GemmXf& xf, float* out);

// def_loss.hip
int launch_def_nearest(hipStream_t st, const float* pred, const float* gold, const float* mask, int B, int N, int64_t* index1, int64_t* index2);
int launch_def_normal_fwd(hipStream_t st, const float* pred, const float* lab, const float* mask, const int64_t* index1, const int64_t* index2, int B,
                          int N, int defpart, float weight, double* part, float* out);
int launch_def_normal_bwd(hipStream_t st, const float* pred, const float* lab, const float* mask, const int64_t* index1, const int64_t* index2, int B,
                          int N, int defpart, float weight, const float* fwd_out, const float* gout, float* dpred);
int launch_def_density_fwd(hipStream_t st, const float* pvec, const float* dens, const float* lvec, const float* lval, const float* mask,
                           const int64_t* index1, const int64_t* index2, int B, int N, int nc, int defpart, float dweight, double* part, float* out);
int launch_def_density_bwd(hipStream_t st, const float* pvec, const float* dens, const float* lvec, const float* lval, const float* mask,
                           const int64_t* index1, const int64_t* index2, int B, int N, int nc, int defpart, float dweight, const float* fwd_out,
                           const float* gkl, const float* gmae, float* dp, float* dd);
int launch_def_gather(hipStream_t st, const uint32_t* x, const int64_t* index, int B, int N, int W, uint32_t* out);
int launch_def_gather_bwd(hipStream_t st, const float* dout, const int64_t* index, int B, int N, int C, float* dx);

// vecattn.hip
size_t vecattn_delta_bwd_ws_floats(int B, int N, int k, int d);       // floats of `part` that launch_vecattn_delta_bwd writes
int launch_vecattn_delta_fwd(hipStream_t st, const float* xyz, int ldx, const int* idx, const float* Wd1, const float* bd1, int B, int N, int k,
                             int d, float* H1);
int launch_vecattn_delta_bwd(hipStream_t st, const float* dH1, const float* H1, const float* xyz, int ldx, const int* idx, int B, int N, int k,
                             int d, float* part, float* dWd1, float* dbd1);
int launch_vecattn_mix_fwd(hipStream_t st, const float* q, int ldq, const float* kk, int ldk, const float* pos, const int* idx, int B, int N, int k,
                           int d, float* T);
int launch_vecattn_mix_bwd(hipStream_t st, const float* dT, int B, int N, int k, int d, float* dq);
int launch_vecattn_aggregate_fwd(hipStream_t st, const float* A, const float* v, int ldv, const float* pos, const int* idx, int B, int N, int k,
                                 int d, float* attn, float* res);
int launch_vecattn_aggregate_bwd(hipStream_t st, const float* dres, const float* attn, const float* v, int ldv, const float* pos, const int* idx,
                                 int B, int N, int k, int d, float* dVP, float* dA);
int launch_vecattn_relu_fwd(hipStream_t st, const float* x, long long rows, int d, float* y);
int launch_vecattn_relu_bwd(hipStream_t st, const float* dy, const float* y, long long rows, int d, float* dx);


// attn.hip
int launch_mhsa_fwd(hipStream_t st, const float* qkv, int ld, int B, int L, int H, int dh, float scale, float* out, float* lse);
int launch_mhsa_bwd(hipStream_t st, const float* qkv, int ld, const float* lse, const float* dout, int B, int L, int H, int dh, float scale,
                    float* dqkv, int ldd);
// a / s / gamma (with beta, y, mean, rstd) nullable: u = x + s[row / rows_per_sample] a;  gamma == NULL writes u only
int launch_layernorm_fwd(hipStream_t st, const float* x, const float* a, const float* s, int rows_per_sample, const float* gamma, const float* beta,
                         long long rows, int d, float eps, float* u, float* y, float* mean, float* rstd);
size_t layernorm_bwd_ws_floats(long long rows, int d);                // floats of `part` that launch_layernorm_bwd writes
// dy NULL: the residual add alone (da = s du; dx, part, dgamma, dbeta untouched);  du / s / dx / da nullable
int launch_layernorm_bwd(hipStream_t st, const float* dy, const float* du, const float* u, const float* s, int rows_per_sample, const float* gamma,
                         const float* mean, const float* rstd, long long rows, int d, float* dx, float* da, float* part, float* dgamma,
                         float* dbeta);
int launch_gelu_fwd(hipStream_t st, const float* x, long long rows, int d, float* y);
int launch_gelu_bwd(hipStream_t st, const float* dy, const float* x, long long rows, int d, float* dx);

// gnedge.hip
size_t gn_edge_ws_bytes(int B, int Nk, int Nq, int k, int C, int groups);   // what the two launchers below take from `ws` (0: shape outside the limits)
int launch_gn_edge_fwd(hipStream_t st, const float* u, int ldu, const float* w, int ldw, const int* idx, const float* gamma, const float* beta,
                       int B, int Nk, int Nq, int k, int C, int groups, float eps, float slope, float* out, uint8_t* argk, float* stats,
                       Workspace& ws);
int launch_gn_edge_bwd(hipStream_t st, const float* dOut, const float* u, int ldu, const float* w, int ldw, const int* idx, const uint8_t* argk,
                       const float* stats, const int* rev_off, const int* rev_ent, const float* gamma, const float* beta, int B, int Nk, int Nq,
                       int k, int C, int groups, float slope, float* du, float* dw, float* dgamma, float* dbeta, Workspace& ws);

// token.hip
size_t thin_in_ws_bytes(int M, int Cin, int C);                             // what the two launchers below take from `ws` (0: shape outside the limits)
// gamma / beta NULL: no BatchNorm;  bias / run_mean / run_var nullable;  xmom [72] doubles (mu | Sigma) is written in training with BatchNorm
int launch_thin_in_fwd(hipStream_t st, const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C, const float* gamma,
                       const float* beta, float* run_mean, float* run_var, float momentum, float eps, int training, int act, float* H,
                       float* bn_save, double* xmom, Workspace& ws);
int launch_thin_in_bwd(hipStream_t st, const float* dH, const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C,
                       const float* gamma, const float* beta, const float* bn_save, const double* xmom, int training, int act, float* dW,
                       float* db, float* dgamma, float* dbeta, Workspace& ws);
int launch_token_pool_fwd(hipStream_t st, const float* y, int B, int L, int d, float* out, int* arg);
int launch_token_pool_bwd(hipStream_t st, const float* dOut, const int* arg, int B, int L, int d, float* dy);

// pyramid.hip
// S == 1: idx / dist / the reverse lists are not read (a broadcast, a cloud sum); S == 2 is refused
int launch_interp3_add_fwd(hipStream_t st, const float* feat, const int* idx, const float* dist, const float* add, int B, int N, int S, int C,
                           float* out);
int launch_interp3_add_bwd(hipStream_t st, const float* dout, const float* dist, const int* rev_off, const int* rev_ent, int B, int N, int S,
                           int C, float* dfeat);
int launch_cloud_mean_fwd(hipStream_t st, const float* X, int B, int N, int C, float* out);
int launch_cloud_mean_bwd(hipStream_t st, const float* dOut, int B, int N, int C, float* dX);

// batchprep.hip
// counts / flags: HOST arrays [B] (nullable); start / Rpre / Rpost / noise: device, nullable where no cloud's flags or count ask for them
int launch_batch_prepare(hipStream_t st, const float* raw, int ld, int B, int Nmax, const int* counts, int S, const int* flags, const int* start,
                         const double* Rpre, const double* Rpost, const double* noise, double sigma, double clip, float* out, int* idx);

// segsup.hip
size_t seg_ws_bytes(int B, int N, int C);                                  // what the two launchers below take from `ws` (0: shape outside the limits)
// loss_pt / mean nullable; stats [B + 1][5] doubles: per cloud loss sum | mIoU | accuracy | valid points | mean loss, row B mean loss | valid points | 0 ..
int launch_seg_ce_fwd(hipStream_t st, const float* logits, int ld, const long long* labels, int B, int N, int C, double* lse, float* loss_pt,
                      long long* pred, double* stats, float* mean, Workspace& ws);
int launch_seg_metrics(hipStream_t st, const long long* labels, const long long* preds, int B, int N, int C, double* stats, Workspace& ws);
// exactly one of g_pt [B N] (reduction 'none') and g_mean [1] (reduction 'mean', with the forward's stats)
int launch_seg_ce_bwd(hipStream_t st, const float* logits, int ld, const long long* labels, const double* lse, int B, int N, int C,
                      const float* g_pt, const float* g_mean, const double* stats, float* dlogits);
