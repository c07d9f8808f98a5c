/* libtxe -- C ABI of the MI355X (gfx950) kernels behind TaxoExpan's propagation / readout / match path.
 *
 * The reference has no FFI of its own: the path sits behind Python classes in model/model_zoo.py that call DGL 0.4
 * and torch.  Each entry point below names the reference lines it replaces; taxoexpan_amd/model_zoo.py binds them
 * with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a BORROWED DEVICE pointer (fp32 / int32, contiguous unless a row stride `ld_*` is given, in
 *     elements); nothing is allocated, freed or synchronised inside; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*);  workspaces are supplied by the caller (size from the *_ws_bytes functions)
 *   - return value: 0 = TXE_OK, <0 = error (TXE_ERR_ARG -1, TXE_ERR_LAUNCH -2, TXE_ERR_WORKSPACE -3); never throws
 *   - re-entrant; no state between calls except the optional per-launch profiler (txe_profile_*, off by default: a process-global
 *     switch and a per-device ring of events) and the cached CU count of the current device
 *   - graph structure: destination-sorted CSR  (rowptr_in[N+1], col_src[E])  and source-sorted CSR
 *     (rowptr_out[N+1], col_dst[E], pos_out[E] = index of that edge in the destination-sorted order); per-edge
 *     arrays (alpha, dz) live in destination-sorted order
 *   - dropout: counter based splitmix64 hash (taxoexpan_amd/csrc/txe_common.h, restated for tests in
 *     taxoexpan_amd/rng.py): features use a precomputed keep-bit mask (txe_dropout_mask), attention coefficients
 *     hash (seed, csr_position*H+head) inline
 */
#ifndef TXE_H
#define TXE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TXE_OK 0
#define TXE_ERR_ARG -1
#define TXE_ERR_LAUNCH -2
#define TXE_ERR_WORKSPACE -3

/* ---- feature dropout (nn.Dropout of model_zoo.py:36,82) as a keep-bit mask over an [n_rows][n_cols] operand: 32 columns per
 * word, ceil(n_cols/32) words per row.  Generated once per layer per step; forward, dX and dW all read the same mask.
 * Pass mask = NULL (or p = 0) to the projections for "no dropout" (eval mode). */
size_t txe_dropout_mask_bytes(long long n_rows, int n_cols);
int txe_dropout_mask(long long n_rows, int n_cols, float p, unsigned long long seed, unsigned* mask, void* stream);

/* ---- GATLayer dense part: model_zoo.py:82-85 (feat_drop, fc, a1, a2) with the PGAT concat of :214-215, on PADDED operands -------
 *   X  [N][Kp]  layer input [h (Kh) | Emb[pos] (Pd) | 0..], Kp = txe_gat_padded_k = roundup(Kh+Pd, 32).  txe_gat_build_x writes it
 *               (h == NULL: the feature part is already in place -- the previous layer's aggregation wrote it -- only the
 *               position-embedding and padding columns are filled).
 *   Wp [Fp][Kp] txe_gat_pack_weights: rows < H*D = fc.weight [H*D][Kh+Pd], rows H*D..H*D+2H = attention projections folded into
 *               the weights (a1 = h (W^T attn_l)), rest 0;  Fp = txe_gat_padded_f = roundup(H*D+2H, 128).
 *   Y  [N][Fp]  = dropout(X) Wp^T = [ft (H*D) | a1 (H) | a2 (H) | unused].
 * txe_gat_dense_bwd: d_Y [N][Fp] in the same layout with ZERO padding columns (txe_zero_cols) -> d_X columns [c0, Kh+Pd)
 * (c0 = 0 if need_dh, else the 4-aligned start of the position columns; columns < Kh x leaky'(X) if act_on -- the backward of
 * the F.leaky_relu of model_zoo.py:216 that produced h -- and all x the dropout factor), dW [H*D][Kh+Pd], d_attn_l/r [H*D],
 * dP [vocab][Pd].  ws: txe_gat_dense_ws_bytes (forward needs only txe_gemm_tail_ws_bytes, or NULL). */
int txe_gat_padded_k(int Kh, int Pd);
int txe_gat_padded_f(int H, int D);
int txe_gat_pack_weights(const float* W, const float* attn_l, const float* attn_r, int H, int D, int Kt, float* Wp, void* stream);
int txe_gat_build_x(const float* h, long long ld_h, int n_nodes, int Kh, const int* pos, const float* P, int Pd, float* X, void* stream);

/* build_x + pack_weights + dropout_mask of one GATLayer (model_zoo.py:80-85) as ONE launch; same outputs as the three calls.
 * mask [n_nodes][ceil((Kh+Pd)/32)] may be NULL when feat_drop_p == 0. */
int txe_gat_layer_prepare(const float* h, long long ld_h, int n_nodes, int Kh, const int* pos, const float* P, int Pd, float* X,
                          const float* W, const float* attn_l, const float* attn_r, int H, int D, float* Wp, float feat_drop_p,
                          unsigned long long seed, unsigned* mask, void* stream);

/* the same for every GATLayer of a stack in ONE launch: a layer's preparation depends on the parameters and on `pos` only, never on the
 * output of the layer below (whose aggregation writes the feature columns of X later), so the whole stack is prepared before its first
 * GEMM.  descs[i]: the arguments of txe_gat_layer_prepare for layer i (h == NULL for every layer but the first). */
struct txe_gat_prepare_desc {
    const float* h; long long ld_h; int n_nodes, Kh; const int* pos; const float* P; int Pd; float* X;
    const float *W, *attn_l, *attn_r; int H, D; float* Wp; float feat_drop_p; unsigned long long seed; unsigned* mask;
    int x_dropped;   /* 1: X is written with the feature dropout already applied -- the layer's GEMMs then take X as a plain operand:
                      * txe_gat_dense_fwd with feat_drop_p = 0 / mask = NULL, txe_gat_dense_bwd with x_dropped = 1 (the mask is still
                      * written: d_X's epilogue needs it).  With h == NULL the producer of the feature columns must drop them itself
                      * (txe_gat_aggregate_fwd with nx_mask and no nx_a12) */
};
int txe_gat_layers_prepare(const struct txe_gat_prepare_desc* descs, int n_layers, void* stream);

/* the same for a GCNLayer (model_zoo.py:35-37): txe_gat_build_x + txe_gcn_pack_weights + txe_dropout_mask as ONE launch */
int txe_gcn_layer_prepare(const float* h, long long ld_h, int n_nodes, int Kh, const int* pos, const float* P, int Pd, float* X,
                          const float* W, int Fo, float* Wp, float drop_p, unsigned long long seed, unsigned* mask, int x_dropped,
                          const float* bias_row /* NULL, or the layer's bias packed as row Kh + Pd of Wp (a padding row must exist) */,
                          void* stream);   /* x_dropped: as in txe_gat_prepare_desc (txe_gcn_dense_fwd then without mask) */
/* ... for every GCNLayer of a stack in ONE launch (descs[i]: the arguments of txe_gcn_layer_prepare for layer i; h == NULL for every layer
 * but the first), together with the stack's norm = in_degree^-1/2 (txe_gcn_norm, model_zoo.py:157-161; rowptr_in == NULL: without it) */
struct txe_gcn_prepare_desc {
    const float* h; long long ld_h; int n_nodes, Kh; const int* pos; const float* P; int Pd; float* X;
    const float* W; int Fo; float* Wp; float drop_p; unsigned long long seed; unsigned* mask; int x_dropped; const float* bias_row;
};
int txe_gcn_layers_prepare(const struct txe_gcn_prepare_desc* descs, int n_layers, const int* rowptr_in, int n_nodes, float* norm, void* stream);

/* Eval-mode layer-0 projection of a batch whose node features are rows of a taxonomy feature table (SURVEY 8f-2 "dedup by _id"):
 * the projection T = table W^T is formed once per DISTINCT taxonomy node (txe_gemm_plain), T2 = the position rows' projections, and
 * every batch node v gets Y[v] = T[row[v]] + T2[row2[v]].  n_cols % 4 == 0, 16-byte aligned rows; T2 / row2 may be NULL. */
int txe_gather_add_rows(const float* T, long long ld_t, const int* row, const float* T2, long long ld_t2, const int* row2, long long n_rows,
                        int n_cols, float* Y, long long ld_y, void* stream);
size_t txe_gat_dense_ws_bytes(int n_nodes, int Kh, int Pd, int H, int D, int vocab);
int txe_gat_dense_fwd(const float* X, int n_nodes, int Kh, int Pd, const float* Wp, int H, int D, float feat_drop_p,
                      const unsigned* mask, float* Y, void* ws, size_t ws_bytes, void* stream);
/* txe_gat_dense_fwd on the bf16 matrix pipe in fp32 accuracy (txe_gemm_nt_split below): X must be a PLAIN operand (dropout already
 * applied -- txe_gat_prepare_desc.x_dropped -- or none).  Xs / Ws = packed planes of X (side 0) / Wp (side 1), or NULL: they are then
 * packed into ws (txe_gat_dense_split_ws_bytes).  Xt_out (or NULL): txe_gat_dense_split_xt_bytes (0 = shape not eligible) for X packed
 * contraction-major (txe_split_pack_t) -- txe_gat_dense_bwd's `Xt`: its weight-gradient product then runs on the same pipe. */
size_t txe_gat_dense_split_ws_bytes(int n_nodes, int Kh, int Pd, int H, int D);
size_t txe_gat_dense_split_xt_bytes(int n_nodes, int Kh, int Pd, int H, int D);
int txe_gat_dense_fwd_split(const float* X, int n_nodes, int Kh, int Pd, const float* Wp, int H, int D, const void* Xs, const void* Ws,
                            void* Xt_out, float* Y, void* ws, size_t ws_bytes, void* stream);
/* ... for a FIRST layer whose input X = dropout([h | Emb[pos]]) (model_zoo.py:82,213-214) is never stored: the packs form its elements
 * from h [N][ld_h], the position table P [vocab][Pd] / pos [N] and the keep mask (NULL or feat_drop_p == 0: no dropout) -- the same
 * planes as packing the stored X, bit for bit.  txe_gat_layers_prepare with desc.X == NULL then writes mask and weights only, and
 * txe_gat_dense_bwd takes X == NULL with Xt (no act_on).  ws: txe_gat_dense_split_ws_bytes. */
int txe_gat_dense_fwd_split_src(const float* h, long long ld_h, const int* pos, const float* P, const unsigned* mask, float feat_drop_p,
                                int n_nodes, int Kh, int Pd, const float* Wp, int H, int D, void* Xt_out, float* Y, void* ws, size_t ws_bytes,
                                void* stream);
int txe_gat_dense_bwd(const float* X, int n_nodes, int Kh, int Pd, const int* pos, int vocab, const float* Wp, const float* W,
                      const float* attn_l, const float* attn_r, int H, int D, float feat_drop_p, const unsigned* mask, const float* d_Y,
                      int need_dh, int act_on, float act_slope, float* d_X, float* dW, float* d_attn_l, float* d_attn_r, float* dP,
                      int x_dropped, const void* Xt, int phases, void* chain, void* ws, size_t ws_bytes, void* stream);
/* phases | TXE_DENSE_DX_SPLIT and need_dh: d_X = d_Y Wp (the whole input gradient of a layer above the first) runs on the bf16 matrix pipe in fp32
 * accuracy, dropout mask and leaky' factor applied in its store loop; its packed operands live behind the workspace:
 * ws_bytes >= txe_gat_dense_ws_bytes + txe_gat_dense_bwd_split_ws_bytes, else TXE_ERR_WORKSPACE.  Without the bit: the fp32 MFMA,
 * whatever the size of the buffer -- the route is the caller's explicit choice. */
size_t txe_gat_dense_bwd_split_ws_bytes(int n_nodes, int Kh, int Pd, int H, int D);
/* phases: TXE_DENSE_ALL = all of it; TXE_DENSE_DX | TXE_DENSE_DW | TXE_DENSE_REDUCE = d_X | the weight-gradient product (split-K partial
 * slices) | the reductions that finish dW, d_attn, dP -- DX and DW are independent, REDUCE needs both.
 * chain (may be NULL): TXE_TAIL_CHAIN_BYTES of HOST memory, zero-filled = empty, owned by the caller for one backward pass.  The last
 * reduction launch of a layer ("phase B": dW / d_attn from the split-K slices, dP, d_pw) only finishes parameter gradients, so a
 * caller may DEFER it with phases | TXE_PH_DEFER: the job is described in the chain instead of launched (its workspace and outputs must
 * stay alive), and the next call WITHOUT the bit that gets the chain -- the bottom layer's -- launches its own phase B and every deferred
 * one together.  txe_gat_tail_flush launches what a chain still holds. */
enum { TXE_DENSE_DX = 1, TXE_DENSE_DW = 2, TXE_DENSE_REDUCE = 4, TXE_DENSE_ALL = 7, TXE_DENSE_DX_SPLIT = 16,
       TXE_PH_DEFER = 64 /* txe_gat_dense_bwd and txe_gat_collapse_bwd_fused */ };
#define TXE_TAIL_CHAIN_BYTES 1024
int txe_gat_tail_flush(void* chain, void* stream);
int txe_zero_cols(float* x, long long ld, int n_rows, int c0, int c1, void* stream);
/* 1 when txe_gat_dense_bwd forms d_X with the streaming position-column kernel (a first PGAT layer: need_dh == 0, the columns behind
 * Kh fit 64 -- model_zoo.py:214-215): TXE_DENSE_DX is then ONE pass over d_Y at HBM speed that also leaves dP's per-class partial sums,
 * and belongs in line on the caller's stream (phases = TXE_DENSE_ALL), not beside the weight-gradient product on a second one. */
int txe_gat_dx_streams(int Kh, int Pd, int need_dh);

/* Eval-mode first GATLayer of a batch whose node features are rows of a feature table (test_fast.py:149-179 / infer.py:82-95
 * encode every taxonomy node many times): the projected rows ft[u] = T[rid[u]] + T2[pos[u]] (T = table x W^T [n_table][ld_t],
 * T2 = position embedding x W_p^T [vocab][ld_t], attention columns at H*D.. as in txe_gat_dense_fwd's output) are formed inside the
 * message/reduce sweep -- same arithmetic as txe_gather_add_rows followed by txe_gat_aggregate_fwd, without the [N][ld_t] round trip.
 * No dropout, alpha is not kept (inference).  nx_*: as in txe_gat_aggregate_fwd (no mask).  _supported: 1 if the shape fits (H <= 4,
 * 16-byte rows, the T2 rows and the folded rows in 56 KB of LDS), else the caller materialises the rows. */
int txe_gat_aggregate_table_supported(int H, int D, long long ld_t, int vocab, int nx_kp);
int txe_gat_aggregate_table_fwd(const int* rowptr_in, const int* col_src, int n_nodes, const float* T, long long ld_t, const int* rid,
                                const float* T2, const int* pos, int vocab, int H, int D, float attn_slope, int out_mode,
                                float act_slope, float* out, long long ld_out, const float* nx_wa, int nx_kp, float* nx_a12,
                                int npw, void* stream);
/* npw: as txe_gat_aggregate_fwd's (0 = chosen from the batch, 1 | 4 = one wave per node, 3 | 8..32 = the egonet walk, forced). */

/* ---- GATLayer message/reduce: model_zoo.py:90-95,106-114 (edge_attention, edge_softmax, attn_drop, update_all) -----
 * out_mode 0: out = aggregated features; 1: out = leaky_relu(aggregated, act_slope) (model_zoo.py:216 fused).
 * alpha [E][H] (post-softmax, pre-dropout; NULL in inference).
 * nx_a12 != NULL (optional fused epilogue, needs 16-byte aligned rows): `out` is the padded input X' [N][nx_kp] of the NEXT, one-head
 * GATLayer (ld_out == nx_kp, its position / padding columns already in place, nx_mask = its feature keep bits or NULL), and the
 * folded attention logits of that layer are formed on the way out: nx_a12[v][r] = <dropout(X'[v]), nx_wa[r]> (nx_wa [2][nx_kp] =
 * rows D, D+1 of its packed weights) -- txe_gat_collapse_fwd then runs with TXE_FOLD_A12_READY.
 * nx_a12 == NULL with nx_mask != NULL and nx_feat_drop_p > 0: `out` is the padded input of the NEXT GATLayer (ld_out == nx_kp, 16-byte
 * rows) and that layer's feature dropout is applied to the rows written (out = dropout(leaky_relu(aggregated))): its GEMMs then read a
 * plain operand (txe_gat_prepare_desc.x_dropped). */
int txe_gat_aggregate_fwd(const int* rowptr_in, const int* col_src, int n_nodes, const float* ft, long long ld_ft,
                          const float* a_src, const float* a_dst, int ld_a, int H, int D, float attn_slope, float attn_drop_p,
                          unsigned long long seed, int out_mode, float act_slope, float* out, long long ld_out, float* alpha,
                          const float* nx_wa, int nx_kp, const unsigned* nx_mask, float nx_feat_drop_p, float* nx_a12, int npw, void* stream);
/* npw: 0 = the sweep is chosen from the batch (batches of 4,096 nodes and more with four heads and 16-byte rows walk egonets:
 * gat_aggregate_ego_kernel, a workgroup per window of consecutive nodes, every row read once); 1 | 2 = one wave per node with that many
 * nodes per wave; 4 = one wave per node, nodes per wave from the batch size; 3 | 8..32 = the egonet walk, forced (with that many nodes per
 * window; TXE_ERR_ARG if the shape does not fit).  `out` and `alpha` are bit-equal across all of them, nx_a12 within rounding (a
 * parity test compares them).
 * d_pre = gradient w.r.t. the PRE-activation aggregated output.  Writes d_ft [N][H*D], d_a_src/d_a_dst [N][H]
 * (row stride ld_da).  dz_ws: E*H floats of scratch.  n_pad: floats following d_a_dst[v][H-1] in every row that are cleared as
 * well (the zero padding columns of txe_gat_dense_bwd's d_Y operand when d_ft | d_a_src | d_a_dst share one padded row); 0 = none. */
int txe_gat_aggregate_bwd(const int* rowptr_in, const int* col_src, const int* rowptr_out, const int* col_dst,
                          const int* pos_out, int n_nodes, const float* ft, long long ld_ft, const float* a_src,
                          const float* a_dst, int ld_a, int H, int D, float attn_slope, float attn_drop_p,
                          unsigned long long seed, const float* alpha, const float* d_pre, long long ld_dpre, float* d_ft,
                          long long ld_dft, float* d_a_src, float* d_a_dst, int ld_da, float* dz_ws, int n_pad, void* stream);
int txe_leaky_relu_bwd(const float* d_out, const float* out_act, float slope, long long n, float* d_pre, void* stream);
/* `.mean(1)` over heads of the output layer, model_zoo.py:219 */
int txe_head_mean_fwd(const float* x, int H, int D, long long n_rows, float* y, void* stream);
int txe_head_mean_bwd(const float* dy, int H, int D, long long n_rows, float* dx, void* stream);

/* ---- GCNLayer: model_zoo.py:34-50 and the norm of :157-161 ------------------------------------------------------ */
/* dense part on padded operands (as for GAT): Wp [roundup(Kp,128)][Fop] = weight [Kt][Fo] zero padded, Fop = roundup(Fo,32) =
 * txe_gcn_padded_f; hw / d_hw [N][Fop] (d_hw with zero padding columns).  txe_gcn_dense_bwd writes d_X [N][Kp] columns [c0,Kt)
 * exactly like txe_gat_dense_bwd, dW [Kt][Fo] and dP [vocab][Pd]. */
int txe_gcn_padded_f(int Fo);
int txe_gcn_pack_weights(const float* W, int Kt, int Fo, float* Wp, void* stream);
size_t txe_gcn_dense_ws_bytes(int n_nodes, int Kh, int Pd, int Fo, int vocab);
int txe_gcn_dense_fwd(const float* X, int n_nodes, int Kh, int Pd, const float* Wp, int Fo, float drop_p, const unsigned* mask,
                      float* hw, void* ws, size_t ws_bytes, void* stream);
int txe_gcn_dense_bwd(const float* X, int n_nodes, int Kh, int Pd, const int* pos, int vocab, const float* Wp, int Fo, float drop_p,
                      const unsigned* mask, const float* d_hw, int need_dh, int act_on, float act_slope, float* d_X, float* dW,
                      float* dP, int x_dropped, void* ws, size_t ws_bytes, void* stream);
int txe_gcn_norm(const int* rowptr_in, int n_nodes, float* norm, void* stream);
int txe_gcn_aggregate_fwd(const int* rowptr_in, const int* col_src, int n_nodes, const float* hw, long long ld_hw,
                          const float* norm, const float* bias, int has_act, float act_slope, int F, float* out, long long ld_out,
                          void* stream);
size_t txe_gcn_aggregate_bwd_ws_bytes(int n_nodes, int F);
int txe_gcn_aggregate_bwd(const int* rowptr_out, const int* col_dst, int n_nodes, const float* d_pre, long long ld_dpre,
                          const float* norm, int F, float* d_hw, long long ld_dhw, float* d_bias, void* ws, size_t ws_bytes,
                          void* stream);   /* also zeroes d_hw's columns [F, min(ld_dhw, roundup(F, 32))): txe_gcn_dense_bwd's zero padding */

/* ---- readouts: MeanReadout model_zoo.py:231-232 (pw = NULL), WeightedMeanReadout :240-242 ------------------------- */
int txe_readout_fwd(const int* graph_off, int G, const float* h, long long ld_h, const int* pos, const float* pw, int D,
                    float* hg, float* wsum, void* stream);
int txe_readout_bwd(const int* graph_off, int G, const float* h, long long ld_h, const int* pos, const float* pw, int vocab,
                    int D, const float* hg, const float* wsum, const float* d_hg, float* d_h, long long ld_dh, float* d_pw,
                    float* dpw_ws, void* stream);

/* SumReadout (mode 1), MaxReadout (mode 2), ConcatReadout (mode 3: [G][3D]) -- model_zoo.py:244-276 */
int txe_readout_multi_fwd(const int* graph_off, int G, const float* h, long long ld_h, const int* pos, int D, int mode, float* hg,
                          int* argmax, void* stream);
int txe_readout_multi_bwd(const int* graph_off, int G, const int* pos, int D, int mode, const float* d_hg, const int* argmax,
                          float* d_h, long long ld_dh, void* stream);

/* AttentionReadout: global attention pooling with a position-aware gate (beyond the reference: its model_zoo.py stops at
 * "TODO: try GlobalAttentionPooling").  Y [N][A] = gate_hidden(h) from txe_linear_fwd, P [vocab][A], u [A]:
 *   s_v = sum_j u_j tanh(Y[v][j] + P[pos_v][j]);  alpha = softmax of s over the egonet (shifted by its maximum);
 *   hg[g] = sum_v alpha_v h[v].   alpha [N] is written once by the forward and read by the backward; an empty egonet gives a zero row.
 * The backward writes d_h = alpha_v d_hg[g] (the term through Y is txe_linear_bwd's), d_Y [N][A], d_P [vocab][A], d_u [A]; it is
 * atomic free: ws (txe_readout_attn_bwd_ws_bytes) holds one [vocab + 1][A] block of column sums per egonet, reduced in a fixed order
 * by a second launch.  vocab <= 8.  G == 0: TXE_OK, nothing launched, nothing written. */
int txe_readout_attn_fwd(const int* graph_off, int G, const float* h, long long ld_h, int D, const float* Y, long long ld_y, int A,
                         const int* pos, const float* P, int vocab, const float* u, float* hg, float* alpha, void* stream);
size_t txe_readout_attn_bwd_ws_bytes(int G, int A, int vocab);
int txe_readout_attn_bwd(const int* graph_off, int G, const float* h, long long ld_h, int D, const float* Y, long long ld_y, int A,
                         const int* pos, const float* P, int vocab, const float* u, const float* hg, const float* alpha,
                         const float* d_hg, long long ld_dhg, float* d_h, long long ld_dh, float* d_Y, long long ld_dy, float* d_P,
                         float* d_u, void* ws, size_t ws_bytes, void* stream);

/* ---- matchers: BIM model_zoo.py:313, LBM :328 (apply_exp) ------------------------------------------------------- */
int txe_bilinear_project(const float* e1, long long ld_e1, int G, int l, const float* W, int r, float* U, long long ld_u,
                         void* sws, size_t sws_bytes, void* stream);   /* sws: NULL, or txe_gemm_plain_split_ws_bytes(G, r, l) of scratch:
                         the product then runs on the bf16 matrix pipe in fp32 accuracy */
int txe_bilinear_pair_fwd(const float* e1, long long ld_e1, const float* e2, long long ld_e2, int G, int l, int r,
                          const float* W, int apply_exp, float* U, float* s, void* stream);
size_t txe_bilinear_pair_bwd_ws_bytes(int G, int l, int r);
int txe_bilinear_pair_bwd(const float* e1, long long ld_e1, const float* e2, long long ld_e2, int G, int l, int r,
                          const float* W, int apply_exp, const float* U, const float* s, const float* ds, float* d_e1,
                          long long ld_de1, float* d_e2, long long ld_de2, float* dW, void* ws, size_t ws_bytes, void* stream);
/* query-side form of the pairwise match for queries that need no gradient (training: model.py:86, trainer.py:51):
 * forward V = E2 W^T [G][l], s_i = <e1_i, V_i> (exp optionally); backward d_e1_i = dsl_i V_i (elementwise -- no second G-row GEMM),
 * dW = (dsl (.) E1)^T E2.  V is kept for backward. */
int txe_bilinear_query_fwd(const float* e1, long long ld_e1, const float* e2, long long ld_e2, int G, int l, int r, const float* W,
                           int apply_exp, float* V, float* s, void* stream);
/* its two halves, for a caller that launches the projection early (it needs the queries and W only) on another stream */
int txe_bilinear_query_project(const float* e2, long long ld_e2, int G, int l, int r, const float* W, float* V, void* stream);
int txe_bilinear_query_dot(const float* e1, long long ld_e1, const float* V, int G, int l, int apply_exp, float* s, void* stream);
size_t txe_bilinear_query_bwd_ws_bytes(int G, int l, int r);
int txe_bilinear_query_bwd(const float* e1, long long ld_e1, const float* e2, long long ld_e2, int G, int l, int r, int apply_exp,
                           const float* V, const float* s, const float* ds, float* d_e1, long long ld_de1, float* dW, void* ws,
                           size_t ws_bytes, void* stream);

/* the pairwise match when the query rows repeat in RUNS: a training batch pairs one query with 1 + negative_size consecutive anchors and
 * data_loaders.py:9-28 stacks that query's row once per pair (trainer.py:46,51 hands the stack to model.py:86).  Qu [U][r] = the
 * distinct rows, run_off [U+1] = first pair of every run (run_off[U] = G): V = Qu W^T [U][l] is U rows instead of G, s_i = <e1_i, V[run(i)]>;
 * backward d_e1_i = dsl_i V[run(i)], dW = S^T Qu with S[u] = sum over run u (pairs in order) of dsl_i e1_i -- K = U instead of G.  Same values
 * as txe_bilinear_query_* on the stacked rows up to the summation order of dW. */
int txe_bilinear_runs_fwd(const float* e1, long long ld_e1, const float* Qu, long long ld_q, const int* run_off, int G, int U, int l, int r,
                          const float* W, int apply_exp, float* V, float* s, void* stream);
size_t txe_bilinear_runs_bwd_ws_bytes(int U, int l, int r);
int txe_bilinear_runs_bwd(const float* e1, long long ld_e1, const float* Qu, long long ld_q, const int* run_off, int G, int U, int l, int r,
                          int apply_exp, const float* V, const float* s, const float* ds, float* d_e1, long long ld_de1, float* dW, void* ws,
                          size_t ws_bytes, void* stream);

/* ... and when the caller only has the reference collate's STACKED matrix E2 [G][r]: txe_rows_find_runs compares every row bit for bit
 * with its predecessor and numbers the runs on the device (run_id [G], run_off [G + 1] with run_off[n_runs] = G, n_runs [1]; no host
 * synchronisation), txe_bilinear_stacked_* are txe_bilinear_runs_* on E2 itself (run u's row = row run_off[u]; V [G][l] and the workspace
 * are sized for G runs, the kernels walk the actual count).  Right for any input; worth it when rows repeat (the caller decides). */
int txe_rows_find_runs(const float* e2, long long ld_e2, int G, int r, int* run_id, int* run_off, int* n_runs, void* stream);
int txe_bilinear_stacked_fwd(const float* e1, long long ld_e1, const float* e2, long long ld_e2, const int* run_off, const int* n_runs, int G,
                             int l, int r, const float* W, int apply_exp, float* V, float* s, void* stream);
size_t txe_bilinear_stacked_bwd_ws_bytes(int G, int l, int r);
int txe_bilinear_stacked_bwd(const float* e1, long long ld_e1, const float* e2, long long ld_e2, const int* run_off, const int* n_runs, int G,
                             int l, int r, int apply_exp, const float* V, const float* s, const float* ds, float* d_e1, long long ld_de1,
                             float* dW, void* ws, size_t ws_bytes, void* stream);

/* The same match FOLDED through the encoder's output layer (model.py:86 on model_zoo.py:313/328 behind :227-242 and the last GATLayer):
 * with hg = Z Wf^T (txe_gat_collapse_fwd, hg == NULL) the score is s_i = <Z_i, T[u(i)]>, T[u] = Wf^T (Wm q_u) -- the D x Kp product runs on
 * the U run rows instead of the G graph rows, forward and backward (dZ_i = dsl_i T[u(i)]; dT[u] = sum dsl_i Z_i; dV = dT Wf^T; dWf = V^T dT,
 * handed to txe_gat_collapse_bwd_fused as dw_main; dWm = dV^T Q).  Runs as in txe_bilinear_runs_* (first_row 0, n_runs NULL, Q = the U
 * distinct rows) or txe_bilinear_stacked_* (first_row 1, the count on the device, U = G sizes V [U][l], T / dT [U][Kp], dV [U][l]). */
int txe_bilinear_folded_fwd(const float* Z, long long ld_z, int G, int Kp, const float* Wf, long long ld_wf, int l, const float* Q, long long ld_q,
                            int r, const int* run_off, const int* n_runs, int U, int first_row, const float* Wm, int apply_exp, float* V, float* T,
                            float* s, int stages /* 1: V and T (queries and weights only), 2: the scores (Z), 3: both */,
                            int wf_by_k /* 0: Wf [l][Kp] (GAT packing); 1: Wf [Kp][ld_wf] (GCN packing), dWf then [Kp][l] */,
                            int one_col /* -1, or the column of Z that counts as 1: row one_col of a by-k Wf holds the layer's bias */, void* stream);
int txe_runs_expand(const int* run_off, int U, int G, int* run_id, void* stream);   /* run_id[i] = the run that holds pair i */
int txe_bilinear_folded_bwd(const float* Z, long long ld_z, int G, int Kp, const float* Wf, long long ld_wf, int l, const float* Q, long long ld_q,
                            int r, const int* run_off, const int* n_runs, int U, int first_row, int apply_exp, const float* V, const float* T,
                            const float* s, const float* ds, float* dZ, long long ld_dz, float* dT, float* dV, float* dWm, float* dWf, int wf_by_k,
                            int one_col, void* stream);

/* nn.Linear over the (virtual) concat of two inputs + activation (0 none / 1 relu / 2 tanh): the MLP matcher, model_zoo.py:285-298 */
int txe_linear_fwd(const float* x1, long long ld1, int l, const float* x2, long long ld2, int r, int G, const float* W, const float* b,
                   int O, int act, float* y, void* stream);
size_t txe_linear_bwd_ws_bytes(int G, int l, int r, int O);
int txe_linear_bwd(const float* x1, long long ld1, int l, const float* x2, long long ld2, int r, int G, const float* W, int O, int act,
                   const float* y, const float* dy, float* dx1, long long ld_dx1, float* dx2, long long ld_dx2, float* dW, float* db,
                   void* ws, size_t ws_bytes, void* stream);
/* ---- all-candidate scoring loop: test_fast.py:116-123 / infer.py:95-99.  U = txe_bilinear_project(hg, W) once, then
 * per query block S[q][g] = match(hg[g], Q[q]) for every candidate g. */
int txe_score_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, int G, int r, int apply_exp, float* S,
                    long long ld_s, void* ws, size_t ws_bytes, void* sws, size_t sws_bytes, const void* u_packed, void* stream);
/* ws: optional, txe_gemm_tail_ws_bytes() of scratch.  sws (here and in the three entry points below; NULL = the fp32 MFMA): scratch of
 * txe_score_split_ws_bytes(nq, G or n_pos, r) bytes -- the product then runs on the bf16 matrix pipe in fp32 accuracy (txe_gemm_nt_split
 * below: Q and U are packed into sws per call) through the SAME epilogues.  The four entry points compare scores bit for bit among
 * themselves: give all of them a workspace or none.
 * u_packed (NULL = pack here): the candidates' planes, txe_split_pack(U, ld_u, G, r, side 1, ...) into txe_split_packed_bytes(G, r) bytes,
 * made ONCE per candidate set -- the loop over query blocks then packs only its queries, and sws needs txe_split_packed_bytes(nq, r)
 * (rounded up to 256) bytes only.  Same planes, same kernel: bit-identical scores either way.
 * TXE_ERR_ARG (all four entry points, before any launch): a negative count, r < 1, ld_u < r, a NULL operand or output, and with more than
 * one query (a single row has no pitch) ld_q < r -- for txe_score_block also ld_s < G; txe_score_topk_block: k < 1, k > 8, G < 1.
 * TXE_ERR_WORKSPACE (before any launch): sws given and sws_bytes too small. */
size_t txe_score_split_ws_bytes(int nq, int G, int r);

/* fused scoring + ranking: the score tile is compared in the GEMM epilogue and never stored.  counts [pos_off[nq]] int32
 * (zeroed by the caller; shards of candidates add) += #{g : score(q, g) strictly better than thr[j]}; thr[j] = score of query q's j-th
 * true parent as computed by txe_score_block (bit-identical k-order).  txe_rank_finalize: ranks[j] = 1 + counts[j] - (the query's
 * other positives that beat j) -- metric.py:7-31. */
int txe_score_count_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, int G, int r, int apply_exp,
                          const int* pos_off, const float* thr, int larger_is_better, int* counts, void* sws, size_t sws_bytes,
                          const void* u_packed, void* stream);
int txe_rank_finalize(const int* pos_off, int nq, const float* thr, const int* counts, int larger_is_better, int* ranks, void* stream);
/* the thresholds themselves: Up [n_pos][r] = the candidate rows of the queries' true parents, query by query (gathered by the caller);
 * thr[j] = match(Q[q], Up[j]) for j in [pos_off[q], pos_off[q+1]) -- the score kernel's own tiles (bit-identical values), but only the
 * tiles along that staircase are computed and only those pairs are stored (test_fast.py:121-123 restricted to rearrange()'s positives) */
int txe_score_positives(const float* Q, long long ld_q, int nq, const float* Up, long long ld_u, int n_pos, int r, int apply_exp,
                        const int* pos_off, float* thr, void* sws, size_t sws_bytes, void* stream);

/* ---- best-k parents of the scoring loop: infer.py:96-106 / test_fast.py:121-131 (`sorted(enumerate(scores), key=...)[:5]`) --------
 * Fused scoring + selection of one query block: no [nq x G] score block is materialised.  Every 128 x 128 tile of the score GEMM
 * (the kernel and k order of txe_score_block: bit-identical scores) leaves each row's k best columns in part_key / part_idx
 * [nq][txe_score_topk_tiles(G)][k] (caller-provided scratch; floor_ws [nq] ints as well: every row's rising selection floor -- a tile
 * skips values below the best k-th key another tile of the row has already secured); txe_topk_merge picks each query's best k: out_idx [nq][k] candidate rows
 * + idx_base (the first row of a candidate shard), best first, -1 where a row has fewer than k candidates; out_key [nq][k] (may be
 * NULL) = the scores, negated when smaller is better.  Order = Python's stable sort: better score first, equal scores by ascending
 * candidate row; NaN ranks last.  1 <= k <= 8.
 * txe_topk_merge alone: best k of `cnt` (key, idx) entries per row (idx == INT_MAX: empty slot; a NaN key counts as -inf) -- also the
 * merge of the per-rank lists of a candidate-sharded loop.  Behind a row's last real entry out_idx is -1 and out_key -inf (as
 * txe_select_k's unused slots), cnt == 0 included: every slot of both outputs is written by every call. */
int txe_score_topk_tiles(int G);
int txe_score_topk_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, int G, int r, int apply_exp,
                         int larger_is_better, int k, int idx_base, float* part_key, int* part_idx, int* floor_ws, int* out_idx,
                         float* out_key, void* sws, size_t sws_bytes, const void* u_packed, void* stream);
int txe_topk_merge(const float* keys, const int* idx, int nq, long long cnt, int k, int idx_base, int* out_idx, float* out_key,
                   void* stream);

/* ---- best-k parents, 9 <= k <= 64: infer.py:96-106 / test_fast.py:121-131 with a longer slice (`sorted(enumerate(scores), key=...)[:k]`:
 * a curator's list of 10 or 20, a re-ranking stage's 50) -- still without the [nq x G] score block.
 * The order is total over (key, column), so a row's best k are its best 8, then the best 8 among the entries strictly worse than the 8th
 * chosen, and so on: ceil(k / 8) rounds of the k <= 8 path (floor initialisation, score tiles, merge), each under a per-row ceiling
 * (key, column) that the round before left -- its last slot as it stands; an empty slot (-inf, INT_MAX) has nothing below it.  One
 * pass of the score tiles per round; the lists, the scratch layout [nq][txe_score_topk_tiles(G)][<= 8] and the k <= 8 entry points are
 * what they were.  Exact and deterministic as they are: the result is a pure function of the scores.
 * txe_score_topk_wide_block: txe_score_topk_block's arguments, order and conventions with 1 <= k <= txe_topk_wide_max() = 64;
 * part_key / part_idx hold [nq][txe_score_topk_tiles(G)][min(k, 8)]; out_idx / out_key [nq][k]; ceil_ws: 8 * nq bytes of scratch ([nq]
 * float keys, then [nq] int columns of this candidate set: idx_base is added on output only).  Every round is enqueued by the one
 * call, nothing is read back; on the bf16 pipe (sws) the operands are packed once.  For k <= 8 the result is txe_score_topk_block's,
 * bit for bit.  TXE_ERR_ARG / TXE_ERR_WORKSPACE before any launch: txe_score_topk_block's rules with k < 1, k > 64, G < 1, a NULL ceil_ws.
 * txe_topk_merge_wide: txe_topk_merge with 1 <= k <= 64 and the same ceil_ws -- the same rounds over given lists (the per-rank lists of
 * a candidate-sharded loop; idx must be distinct within a row).  TXE_ERR_ARG: nq < 0, cnt < 0, k < 1, k > 64, a NULL keys / idx / out_idx /
 * ceil_ws. */
int txe_topk_wide_max(void);
int txe_score_topk_wide_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, int G, int r, int apply_exp,
                              int larger_is_better, int k, int idx_base, float* part_key, int* part_idx, int* floor_ws, int* out_idx,
                              float* out_key, void* sws, size_t sws_bytes, const void* u_packed, void* ceil_ws, void* stream);
int txe_topk_merge_wide(const float* keys, const int* idx, int nq, long long cnt, int k, int idx_base, int* out_idx, float* out_key,
                        void* ceil_ws, void* stream);

/* ---- log-partition of the scoring loop: model/loss.py:52-57 (info_nce_loss: F.cross_entropy over [positive | sampled negatives]) over
 * test_fast.py:121-123 / infer.py:97-99 (the scores of ALL candidates) -- the exact denominator of p(a | q) = exp(z(q, a)) / sum_a' exp(z(q, a')).
 * Fused scoring + reduction of one query block: no [nq x G] score block is materialised.  s = the score kernel's own value (the kernel
 * and k order of txe_score_block: bit-identical), z = s when larger_is_better, else -s;
 *     lse[q] = log sum_{g < G} exp(z[q][g])    as the IEEE value of the float64 formula on the fp32 scores:
 * a NaN score in the row gives NaN; otherwise a z = +Inf gives +Inf; otherwise all z = -Inf gives -Inf; otherwise M + log sum exp(z - M),
 * M = max z (a lone candidate, or a leader the rest vanish beside, gives M bit for bit).  Every 128 x 128 tile of the score GEMM leaves, per
 * row, (max z, sum exp(z - max)) over its columns < G in part_max / part_sum [nq][txe_score_topk_tiles(G)] (caller-provided scratch,
 * rewritten by every call; an empty or all -Inf part is (-Inf, 0), a part with NaN / +Inf carries it as its max); txe_lse_merge
 * combines a row's pairs in float64, tiles in a fixed order, no atomics: lse[q] is a function of row q's scores alone -- the same bits
 * whatever the block size, the row's place in the block, or the run.  The three routes of txe_score_block (fp32 MFMA with sws = NULL, the
 * bf16 pipe packed per call, u_packed) give the same bits wherever their scores are.
 * TXE_ERR_ARG / TXE_ERR_WORKSPACE before any launch, as txe_score_topk_block: a negative count, G < 1, r < 1, ld_u < r, a NULL operand,
 * scratch or output, with more than one query ld_q < r; sws given and sws_bytes too small.  nq == 0: TXE_OK, nothing launched.
 * txe_lse_merge alone: lse [nq] from `cnt` (max, sum) pairs per row ([nq][cnt]) -- also the merge of the per-rank pairs of a
 * candidate-sharded loop.  cnt == 0: every lse is -Inf.  TXE_ERR_ARG: nq < 0, cnt < 0, a NULL pointer. */
int txe_score_lse_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, int G, int r, int apply_exp,
                        int larger_is_better, float* part_max, float* part_sum, float* lse, void* sws, size_t sws_bytes,
                        const void* u_packed, void* stream);
int txe_lse_merge(const float* part_max, const float* part_sum, int nq, long long cnt, float* lse, void* stream);

/* ---- moments of the predictive distribution (calibration): the lse mode above under a score scale beta = 1 / temperature, with the first
 * two moments of the scaled score.  For a query row with candidates g < G:
 *     s = the score kernel's own value (bit-identical to txe_*_score_block, exp applied where apply_exp is set),
 *     z = s when larger_is_better, else -s,
 *     t = fl32(beta * z): ONE fp32 multiply, rounded before anything else uses it (never contracted into the subtraction of the maximum);
 * beta is fp32, finite and > 0.  A set of candidates (one tile's columns of a row, or the whole row) is carried as the quadruple
 *     m = max t (NaN kept),   s0 = sum exp(d),   s1 = sum d exp(d),   s2 = sum d^2 exp(d),      d = t - m <= 0
 * -- sums centred at the set's own maximum: nothing overflows and E[t^2] - E[t]^2 is never formed from large numbers.  A candidate with
 * t = -Inf adds nothing to any sum (no -Inf * 0); s0 / s1 / s2 count only while m is finite.  A row's quadruples merge in float64, parts in
 * a fixed order, no atomics: with M = max m_i, delta_i = m_i - M, w_i = exp(delta_i)
 *     S0 = sum w s0,   S1 = sum w (s1 + delta s0),   S2 = sum w (s2 + 2 delta s1 + delta^2 s0)
 *     lse = M + log S0,   mean = M + S1 / S0,   var = max(S2 / S0 - (S1 / S0)^2, 0),   entropy = max(log S0 - S1 / S0, 0)
 * (a part more than 104 below M -- where fp32's exp is exactly 0 -- adds nothing to S1 and S2, as a candidate that far behind adds nothing
 * inside a tile).  mean = E_p[t], var = Var_p[t], entropy = H(p), p = softmax(t); d lse / d beta = mean / beta, d^2 lse / d beta^2 =
 * var / beta^2.  entropy comes from S0 and S1, not from lse - mean, which cancels for a peaked row.  out: float64 [nq][4] in that order.
 * lse follows txe_score_lse_block's rules exactly (NaN in the row: NaN; else a +Inf: +Inf; else all -Inf: -Inf), and at beta = 1
 * (float)lse has txe_*_score_lse_block's bits; wherever lse is not finite, mean, var and entropy are NaN.  G = 1: entropy = var = 0 and
 * mean = (double)t; a leader more than 110 ahead of the rest after scaling: entropy = 0 and mean = M.  A row's four values depend on the
 * row's scores and beta alone: not on the block size, the row's place in the block, the route, or the run.
 * part_max / part_s0 / part_s1 / part_s2: [nq][txe_score_topk_tiles(G)] caller-provided scratch, rewritten by every call.
 * TXE_ERR_ARG / TXE_ERR_WORKSPACE before any launch: txe_score_lse_block's rules, beta not finite or <= 0, a NULL scratch or output.
 * nq == 0: TXE_OK, nothing launched.  The MLP and NTN forms mirror their lse entry points.
 * txe_moments_merge alone: out [nq][4] from `cnt` quadruples per row ([nq][cnt] each) -- also the merge of the per-rank quadruples of a
 * candidate-sharded loop.  cnt == 0: lse = -Inf, the other three NaN.  TXE_ERR_ARG: nq < 0, cnt < 0, a NULL pointer. */
int txe_score_moments_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, int G, int r, int apply_exp,
                            int larger_is_better, float beta, float* part_max, float* part_s0, float* part_s1, float* part_s2, double* out,
                            void* sws, size_t sws_bytes, const void* u_packed, void* stream);
int txe_mlp_score_moments_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                                const float* mw, int larger_is_better, float beta, float* part_max, float* part_s0, float* part_s1,
                                float* part_s2, double* out, void* stream);
int txe_ntn_score_moments_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                                const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, int larger_is_better,
                                float beta, float* part_max, float* part_s0, float* part_s1, float* part_s2, double* out, void* stream);
int txe_moments_merge(const float* part_max, const float* part_s0, const float* part_s1, const float* part_s2, int nq, long long cnt,
                      double* out, void* stream);

/* ---- retrieval stage of the two-stage test protocol (data_loader/dataset.py:316-330; csrc/txe_retrieve.hip) -------------------------
 * txe_row_normalize: y[i] = x[i] / ||x[i]||_2 (fp32, any pitch, y apart from x): cosine similarity then is a plain dot product, formed by
 * txe_score_block with apply_exp = 0.  A zero-norm or non-finite row becomes NaN and gives NaN similarities.
 * txe_select_k: out_idx [nq][k] = per row of S [nq][G] (pitch ld_s; never written) the k columns with the largest value that the row's
 * mask list does not name, best first, equal values by ascending column, NaN last (NaN takes the place of -inf; -0.0 == +0.0) -- the
 * order of txe_topk_merge; -1 where the row has fewer than k unmasked columns.  out_key [nq][k] (may be NULL) = those values (NaN as
 * -inf; -inf in the unused slots).  Masks: CSR, row q masks the columns mask_idx[mask_off[q] .. mask_off[q+1]) (any order, duplicates
 * and empty lists allowed, a column outside [0, G) names nothing); both NULL = no masks.  With masks ws holds
 * txe_select_k_ws_bytes(nq, G) bytes (a bitmap, rewritten by every call), else TXE_ERR_WORKSPACE; without, ws may be NULL.
 * One workgroup per row, integer histograms and a sort on distinct keys: the result is a pure function of S and the masks.
 * TXE_ERR_ARG (before any device work): k < 1 or k > 4096, a NULL S / out_idx, one of mask_off / mask_idx without the other, nq < 0,
 * G < 1, ld_s < G. */
int txe_row_normalize(const float* x, long long ld_x, int n, int d, float* y, long long ld_y, void* stream);
size_t txe_select_k_ws_bytes(int nq, int G);
int txe_select_k(const float* S, long long ld_s, int nq, int G, const int* mask_off, const int* mask_idx, int k, int* out_idx, float* out_key,
                 void* ws, size_t ws_bytes, void* stream);

/* ---- all-candidate scoring loop of the MLP matcher (model_zoo.py:285-298 under test_fast.py:121-123 / infer.py:97-99) ---------------
 * W1 = ffn[0].weight [H][l+r] = [W1a | W1b], b1, w2 = ffn[2].weight [H], b2 = ffn[2].bias [1].  A = hg W1a^T + b1 [G][H] comes from
 * txe_linear_fwd (x2 = NULL); then S[q][g] = b2 + sum_h w2[h] relu(A[g][h] + B[q][h]), B = Qf W1b^T, is evaluated on the VALU as
 * c[q] + sum_h w2[h] max(A[g][h], -B[q][h]) with c[q] = b2 + sum_h w2[h] B[q][h] (one max + one FMA per pair and h; h ascending, never
 * split: every mode below sees bit-identical scores).  Rows of A or B holding NaN / +-Inf / |x| > lim = 2^120 / max(1, sum |w2|) are
 * flagged and their pairs take the literal formula (NaN propagates through relu as in torch).  Hp = txe_mlp_padded_h(H) (a multiple of
 * 16): A, -B and w2 are zero-padded to it.
 * txe_mlp_project: Ap [G][Hp] = A padded, flag_a [G], mw [Hp + 2] = (w2 padded, b2, lim) -- once per candidate set (G may be 0: mw only).
 * txe_mlp_query_project: per query block, W1bT [r][H] = W1b transposed: nB [nq][Hp] = -B padded, c [nq], flag_b [nq].
 * The four scoring entry points mirror txe_score_block / txe_score_positives / txe_score_count_block / txe_score_topk_block (same
 * pos_off / thr / counts / part_key / part_idx / floor_ws conventions; the top-k tiles are 128 candidates wide: txe_score_topk_tiles(G));
 * positives take the candidate rows directly (pos_idx [n_pos]; a row outside [0, G) gives 0: a positive of another shard). */
int txe_mlp_padded_h(int H);
int txe_mlp_project(const float* A, long long ld_a, int G, int H, const float* w2, const float* b2, float* Ap, float* mw, int* flag_a,
                    void* stream);
int txe_mlp_query_project(const float* Qf, long long ld_q, int nq, int r, const float* W1bT, int H, const float* mw, float* nB, float* c,
                          int* flag_b, void* stream);
int txe_mlp_score_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                        const float* mw, float* S, long long ld_s, void* stream);
int txe_mlp_score_positives(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                            const float* mw, const int* pos_off, const int* pos_idx, int n_pos, float* thr, void* stream);
int txe_mlp_score_count_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                              const float* mw, const int* pos_off, const float* thr, int larger_is_better, int* counts, void* stream);
int txe_mlp_score_topk_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                             const float* mw, int larger_is_better, int k, int idx_base, float* part_key, int* part_idx, int* floor_ws,
                             int* out_idx, float* out_key, void* stream);
/* model_zoo.py:285-298 under infer.py:100-106 with a longer slice -- txe_mlp_score_topk_block for 1 <= k <= 64: txe_score_topk_wide_block's
 * rounds, scratch (part_key / part_idx [nq][txe_score_topk_tiles(G)][min(k, 8)], ceil_ws 8 * nq bytes) and refusals; k <= 8 bit-equal
 * to txe_mlp_score_topk_block */
int txe_mlp_score_topk_wide_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                                  const float* mw, int larger_is_better, int k, int idx_base, float* part_key, int* part_idx,
                                  int* floor_ws, int* out_idx, float* out_key, void* ceil_ws, void* stream);
/* model_zoo.py:285-298 under model/loss.py:52-57 over test_fast.py:121-123 / infer.py:97-99 -- the log-partition of every query over all
 * candidates, txe_score_lse_block's definition, scratch and merge (the pair kernel's tiles are 128 candidates wide too).
 * TXE_ERR_ARG before any launch: the four entry points' rules, G < 1, a NULL part_max / part_sum / lse.  nq == 0: TXE_OK, no launch. */
int txe_mlp_score_lse_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                            const float* mw, int larger_is_better, float* part_max, float* part_sum, float* lse, void* stream);

/* ---- all-candidate scoring loop of the NTN matcher (model_zoo.py:331-346 under test_fast.py:121-123 / infer.py:97-99) ---------------
 * W = W.weight [k][l][r], b = W.bias [k], V = V.weight [k][l+r] = [V1 | V2], u = u_R.weight [k].  For candidate g, query q, slice j < k:
 *     S[q][g] = sum_j u_j tanh((<q, U_j[g]> + a_j[g]) + c_j[q]),   U_j = hg W_j,   a_j[g] = V1_j . hg[g] + b_j,   c_j[q] = V2_j . q
 * 1 <= k <= 16.  The U_j come from txe_bilinear_project: once per slice, or in one call on the stacked weight [l][k * rp] -- slice j of
 * candidate g then lies at U + g * ld_u + j * slice_u.  The pair work is the score GEMM's 128 x 128 tile (csrc/txe_ntn_score.hip: fp32
 * MFMA, full k order, never split along the reduction) run once per slice inside one workgroup, each slice folded into the tile by
 * s = fma(u_j, tanh((acc + a_j[g]) + c_j[q]), s); the finished tile goes to the score GEMM's own epilogue.  No [nq][G][k] tensor is
 * written; every mode below sees bit-identical scores, and a score is a function of its two rows' values only.  tanh: relatively
 * accurate down to zero, exactly +-1 where it saturates (+-Inf included), NaN for NaN.
 * The four scoring entry points mirror txe_score_block / txe_score_positives / txe_score_count_block / txe_score_topk_block: the same
 * pos_off / thr / counts / part_key / part_idx / floor_ws / idx_base conventions, the same txe_score_topk_tiles(G); positives take the
 * GATHERED candidate side (U and a of the queries' true parents, query by query: G = n_pos) like txe_score_positives.
 * a is [k][G] on pitch ld_a, c is [k][nq] on pitch ld_c (slice-major: a tile reads 128 consecutive floats per slice).
 * TXE_ERR_ARG before any device work: k < 1 or k > 16, r < 1 (l < 1), a negative size, a pitch below its width (ld_u < r, slice_u < r,
 * ld_q < r for more than one query, ld_a < G, ld_c < nq, ld_s < G), a NULL required pointer, a top-k size outside 1..8 (or G < 1 there).
 * TXE_OK without a launch when nq == 0 or G == 0. */
/* model_zoo.py:331-346, test_fast.py:121-123 -- candidate side, once per candidate set: a [k][G] from hg [G][l], V1 (rows of V.weight, pitch
 * ld_v = l + r) and b */
int txe_ntn_project(const float* hg, long long ld_hg, int G, int l, const float* V1, long long ld_v, const float* b, int k, float* a,
                    long long ld_a, void* stream);
/* model_zoo.py:331-346, test_fast.py:121-123 -- query side, per query block: c [k][nq] from Q [nq][r] and V2 = V.weight + l (pitch ld_v) */
int txe_ntn_query_project(const float* Q, long long ld_q, int nq, int r, const float* V2, long long ld_v, int k, float* c, long long ld_c,
                          void* stream);
/* model_zoo.py:331-346, test_fast.py:121-123 -- S [nq][G] (pitch ld_s) */
int txe_ntn_score_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                        const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, float* S, long long ld_s,
                        void* stream);
/* model_zoo.py:331-346, test_fast.py:121-123 -- thr[j] = S[q][j] for j in [pos_off[q], pos_off[q+1]) over the gathered candidate side */
int txe_ntn_score_positives(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                            const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, const int* pos_off,
                            float* thr, void* stream);
/* model_zoo.py:331-346, test_fast.py:121-123 -- counts[j] += #{g < G : S[q][g] strictly better than thr[j]} */
int txe_ntn_score_count_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                              const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, const int* pos_off,
                              const float* thr, int larger_is_better, int* counts, void* stream);
/* model_zoo.py:331-346, test_fast.py:121-123 / infer.py:100-106 -- the best `topk` candidates per query, in txe_score_topk_block's order */
int txe_ntn_score_topk_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                             const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, int larger_is_better,
                             int topk, int idx_base, float* part_key, int* part_idx, int* floor_ws, int* out_idx, float* out_key,
                             void* stream);
/* model_zoo.py:331-346, test_fast.py:121-123 / infer.py:100-106 with a longer slice -- txe_ntn_score_topk_block for 1 <= topk <= 64:
 * txe_score_topk_wide_block's rounds, scratch (part_key / part_idx [nq][txe_score_topk_tiles(G)][min(topk, 8)], ceil_ws 8 * nq bytes) and
 * refusals; topk <= 8 bit-equal to txe_ntn_score_topk_block */
int txe_ntn_score_topk_wide_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                                  const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k,
                                  int larger_is_better, int topk, int idx_base, float* part_key, int* part_idx, int* floor_ws, int* out_idx,
                                  float* out_key, void* ceil_ws, void* stream);
/* model_zoo.py:331-346 under model/loss.py:52-57 over test_fast.py:121-123 / infer.py:97-99 -- the log-partition of every query over all
 * candidates, txe_score_lse_block's definition, scratch and merge.  TXE_ERR_ARG before any launch: the four entry points' rules, G < 1,
 * a NULL part_max / part_sum / lse.  nq == 0: TXE_OK, no launch. */
int txe_ntn_score_lse_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                            const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, int larger_is_better,
                            float* part_max, float* part_sum, float* lse, void* stream);

/* plain dense product on the fp32 MFMA GEMM (tests / micro-benchmarks).  layout 0: C = A[M][K] B[N][K]^T; 1: C = A[M][K] B[K][N];
 * 2: C = A[K][M]^T B[K][N].  splits > 1: `splits` partial products at C + z*M*ldc.  ws/ws_bytes (optional, txe_gemm_tail_ws_bytes):
 * scratch that lets the last, partial round of workgroups be split along k ("tail splitting").
 * route: 0 = the route the model paths take; test bits selecting a bit-equal alternative kernel: 1 = whole rounds on gemm_kernel instead
 * of the persistent kernel, 2 = split-K TN products without the LDS-direct copies, 4 = every eligible split-K product on 128 x 160 tiles.
 * route bit 8 (layout 0, splits 1): the product runs on the bf16 matrix pipe in fp32 accuracy (txe_gemm_nt_split below); ws then holds the
 * packed operands -- txe_gemm_plain_split_ws_bytes(M, N, K) bytes. */
size_t txe_gemm_tail_ws_bytes(void);
size_t txe_gemm_plain_split_ws_bytes(int M, int N, int K);
int txe_gemm_plain(int layout, const float* A, long long lda, const float* B, long long ldb, float* C, long long ldc, int M, int N,
                   int K, int splits, int route, void* ws, size_t ws_bytes, void* stream);

/* ---- rank extraction of the scoring loop: test_fast.py:16-22 + model/metric.py:7-31 (strict inequalities, the
 * query's other positives excluded).  pos_off [nq+1], pos_idx: candidate columns of each query's true parents. */
int txe_rank_block(const float* S, long long ld_s, int nq, int G, const int* pos_off, const int* pos_idx, int* ranks,
                   int larger_is_better, void* ws_unused, void* stream);

/* ---- graph structure: the batched-egonet COO of dgl.batch (data_loaders.py:25; edge order dataset.py:431-435) to the
 * two CSR views the kernels read (stable: in-edges stay in edge-id order). */
size_t txe_build_csr_ws_bytes(int n_nodes, int n_edges);
int txe_build_csr(const int* src, const int* dst, int n_nodes, int n_edges, int* rowptr_in, int* col_src, int* eid_in,
                  int* rowptr_out, int* col_dst, int* pos_out, void* ws, size_t ws_bytes, void* stream);

/* ---- output GATLayer (ONE head) folded behind MeanReadout / WeightedMeanReadout: model_zoo.py:80-104,219,227-242.
 * hg[g] = (sum_{u in g} c_u Xd[u]) W^T with c_u = sum_{v: u->v} w_v alpha'_uv / S_g -- the same arithmetic as projection ->
 * edge-softmax aggregation -> weighted mean, re-associated so that the projection and its dX / dW products run on G graph rows
 * instead of N node rows.  X [N][Kp] / Wp [Fp][Kp] / mask as for txe_gat_dense_*; pw == NULL: MeanReadout.  Forward keeps
 * a12 [N][2], alpha [E], coef [N], wsum [G], gid [N], Z [G][Kp] for backward; d_X has the layout txe_gat_dense_bwd produces. */
size_t txe_gat_collapse_ws_bytes(int n_nodes, int n_edges, int G, int Kh, int Pd, int D, int vocab);
/* ws_bytes >= txe_gat_collapse_ws_bytes + txe_gat_collapse_split_ws_bytes: txe_gat_collapse_fwd forms hg = Z W^T on the bf16 matrix pipe in
 * fp32 accuracy (txe_gemm_nt_split below) */
size_t txe_gat_collapse_split_ws_bytes(int G, int Kh, int Pd, int D);
/* The arguments of the folded-layer entry points, grouped by what they are; every fact lives in one struct.  Plain structs of borrowed
 * device pointers and scalars: the caller keeps what they point to alive and may fill them once per forward pass for all the calls of a step. */
struct txe_graph_batch {       /* the batch of graphs: both CSR orders, graph_off [G + 1] = first node of every graph */
    const int *rowptr_in, *col_src, *rowptr_out, *col_dst, *pos_out, *graph_off; int n_nodes, n_edges, G;
};
struct txe_gat_fold_layer {    /* the folded GAT layer: its inputs, then what forward writes and the backward calls read */
    const float* X; int Kh, Pd; const int* pos; int vocab /* backward only */; const float *Wp, *W, *attn_l, *attn_r /* W, attn_*: backward only */;
    int D; float feat_drop_p; const unsigned* mask; float attn_slope, attn_drop_p; unsigned long long seed; const float* pw;
    float *a12, *alpha, *coef, *wsum; int* gid; float *Z, *hg; long long ld_hg;   /* hg NULL: forward stops at Z (the consumer folds hg = Z W^T) */
};
struct txe_fold_match {        /* the folded matcher's share (txe_bilinear_folded_*): Tf [runs][Kp], zrow [G] graph -> its row of Tf, e_part
                                * [N][txe_gat_collapse_e_tiles]; backward adds the matcher's score gradient m_ds [G], its scores m_s [G], whether it
                                * exponentiates, and zgid [N] scratch.  A NULL struct (or NULL pointers in it): no matcher rides along */
    float* e_part; const float *m_ds, *m_s; int m_exp; const float* Tf; const int* zrow; int* zgid;
};
/* flags: A12_READY: a12 holds the logits already; HG_SPLIT: hg = Z W^T on the bf16 matrix pipe -- ws_bytes >= txe_gat_collapse_ws_bytes +
 * txe_gat_collapse_split_ws_bytes, else TXE_ERR_WORKSPACE. */
enum { TXE_FOLD_A12_READY = 1, TXE_FOLD_HG_SPLIT = 2 };
/* match (may be NULL; needs layer->hg == NULL): Tf, zrow and e_part all given -- see TXE_FUSED_EDOT below */
int txe_gat_collapse_fwd(const struct txe_graph_batch* batch, const struct txe_gat_fold_layer* layer, const struct txe_fold_match* match,
                         int flags, void* ws, size_t ws_bytes, void* stream);
int txe_gat_collapse_e_tiles(int n_nodes, int G, int Kh, int Pd);   /* floats per node of e_part; 0: this batch cannot form it */
/* the folded matcher's scores from e_part: s_g = [exp] <Z_g, Tf[zrow[g]]> = [exp] (scale / S_g) sum_{u in g} coef_u e_u -- no sweep over Z
 * (masked: the layer's keep mask was applied, i.e. scale = 1 / (1 - feat_drop_p)) */
int txe_gat_collapse_fold_scores(const int* graph_off, int n_nodes, int G, int Kh, int Pd, const float* coef, const float* wsum, const float* e_part,
                                 float feat_drop_p, int masked, int apply_exp, float* s, void* stream);
struct txe_gat_fold_grads { float *dW, *d_attn_l, *d_attn_r, *dP, *d_pw; };   /* the folded layer's parameter gradients */
int txe_gat_collapse_bwd(const struct txe_graph_batch* batch, const struct txe_gat_fold_layer* layer, const float* d_hg, long long ld_dhg,
                         int act_on, float act_slope, float* d_X, const struct txe_gat_fold_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* txe_gat_collapse_bwd FUSED with txe_gat_aggregate_bwd of the GATLayer below it (one HBM sweep instead of three): the
 * gradient of the folded layer's input is formed on the fly from X, dZ and the attention-logit gradients while the layer below's
 * source-side sweep runs, and never stored.  Extra inputs: that layer's projection output Yp [N][ld_yp] = [ft | a1 | a2] (Hp heads x
 * Dp, Hp*Dp == Kh), its attention alpha_p [E][Hp] (destination-CSR order), slope / dropout / seed (struct txe_gat_fold_below), the slope of
 * the activation between the layers (act_slope, 1 = none).  Output instead of d_X: d_Yp [N][ld_dyp] = [d_ft | d_a1 | d_a2 | n_pad zeros];
 * dz_p [E][Hp] scratch.
 * phases: TXE_FUSED_ALL = all of it; TXE_FUSED_DZ | _DW | _SWEEP | _REDUCE = dZ GEMM | dW GEMM partials (independent of DZ and SWEEP: a
 * second stream may run it under the sweeps) | sweeps + first reduction stage (needs DZ) | final reductions (needs DW and SWEEP) --
 * separate calls share the workspace; TXE_FUSED_REDUCE | TXE_PH_DEFER with a chain defers the final reductions (see txe_gat_dense_bwd).
 * | TXE_FUSED_DW_BESIDE (on EVERY call of one backward pass: the workspace layout depends on it): the dW product runs beside other
 * kernels on a second stream and is cut into at most 2 fat k-slices, which leave those kernels their wave slots.
 * | TXE_FUSED_DZ_GIVEN: the caller folded hg = Z W^T into the consumer of Z (txe_bilinear_folded_*; txe_gat_collapse_fwd with hg == NULL
 * stops at Z): `d_hg` IS dZ [G][Kp] (ld_dhg == Kp), hg may be NULL, DZ and DW do not run, and the main part of dW comes from the caller
 * as dw_slices slices [D][Kp] at dw_main (summed in order; 0 slices: none) -- this call adds the attention rows' part.
 * | TXE_FUSED_EDOT (with DZ_GIVEN): the <dZ, X> sweep was formed in forward -- txe_gat_collapse_fwd with a txe_fold_match leaves
 * <Tf[zrow[g]], keep X[u]> in e_part; with the folded matcher's dZ[g] = dsl_g Tf[zrow[g]] backward needs only the rest of that struct:
 * the fused sweep reads its "dZ[g]" rows as Tf[zrow[g]] with dsl_g folded into the node coefficients -- d_hg may be NULL, dZ is never
 * formed.
 * | TXE_FUSED_NO_EGO_WALK: the source-side sweep does not walk egonets from registers, whatever the head count (the A/B switch).
 * | TXE_WALK_NO_REFORM: the egonet walk (Hp == 4) loads the X rows of parents and siblings.  Without the bit it forms their feature
 * columns again from Yp, alpha_p and the dropout seed -- bit-identical, and a quarter of the sweep's reads less -- which REQUIRES that
 * X's columns [0, Kh) are what txe_gat_aggregate_fwd wrote for this Yp / alpha_p with out_mode 1 and act_slope (or out_mode 0 and
 * act_slope 1), not the dropped form its nx_kp > 0 && nx_a12 == NULL call stores.  A caller that cannot vouch for that sets the bit.
 * txe_gat_fused_bwd_supported: 1 if the shape qualifies (Hp in {1,2,4}, Hp*Dp % 16 == 0, <= 128 columns behind the feature part). */
int txe_gat_fused_bwd_supported(int Kh, int Pd, int Hp, int Dp);
size_t txe_gat_collapse_bwd_fused_ws_bytes(int n_nodes, int n_edges, int G, int Kh, int Pd, int D, int vocab, int Hp);
enum { TXE_FUSED_DZ = 1, TXE_FUSED_DW = 2, TXE_FUSED_SWEEP = 4, TXE_FUSED_REDUCE = 8, TXE_FUSED_ALL = 15, TXE_FUSED_DW_BESIDE = 128,
       TXE_FUSED_DZ_GIVEN = 256, TXE_FUSED_EDOT = 512, TXE_FUSED_NO_EGO_WALK = 1024 };
enum { TXE_WALK_NO_REFORM = 2048 };    /* a `phases` bit of txe_gat_collapse_bwd_fused like the ones above: how the egonet walk gets its rows */
struct txe_gat_fold_below {    /* the GATLayer below the folded one */
    const float* Yp; long long ld_yp; int Hp, Dp; float attn_slope_p, attn_drop_p_p; unsigned long long seed_p; const float* alpha_p;
    float* d_Yp; long long ld_dyp; int n_pad; float* dz_p;
};
int txe_gat_collapse_bwd_fused(const struct txe_graph_batch* batch, const struct txe_gat_fold_layer* layer, const struct txe_gat_fold_below* below,
                               const struct txe_fold_match* match /* NULL without TXE_FUSED_EDOT */, const struct txe_gat_fold_grads* grads,
                               const float* d_hg, long long ld_dhg, float act_slope, int phases, const float* dw_main, int dw_slices,
                               const int* walk_plan, void* chain, void* ws, size_t ws_bytes, void* stream);
/* walk_plan (optional, NULL = none): the batch's plan from txe_egonet_walk_plan -- what the egonet-walking sweep otherwise works out from
 * the CSR arrays in every workgroup of every step (hub, roles, CSR positions, list order of each graph) done once per batch of graphs:
 * the sweep's staging is then two dependent trips instead of eight.  Same results bit for bit.  plan: txe_egonet_walk_plan_bytes(n_nodes)
 * bytes, 16-byte aligned; depends on the graphs only (both CSR orders, graph offsets), valid as long as they are. */
size_t txe_egonet_walk_plan_bytes(int n_nodes);
int txe_egonet_walk_plan(const int* rowptr_in, const int* col_src, const int* rowptr_out, const int* col_dst, const int* pos_out,
                         const int* graph_off, int n_nodes, int G, int* plan, void* stream);

/* ---- output GCNLayer folded behind MeanReadout / WeightedMeanReadout: model_zoo.py:35-47,139-167,227-242.
 * hg[g] = (sum_{u in g} c_u Xd[u]) W + b with c_u = norm_u sum_{v: u->v} w_v norm_v / S_g (graph constants).  X / Wp / mask as for
 * txe_gcn_dense_*; norm from txe_gcn_norm; forward keeps coef [N], wsum [G], gid [N], Z [G][Kp]. */
size_t txe_gcn_collapse_ws_bytes(int n_nodes, int G, int Kh, int Pd, int Fo, int vocab);
struct txe_gcn_fold_layer {    /* the folded GCN layer (the batch is a txe_graph_batch; pos_out and n_edges are not read) */
    const float* X; int Kh, Pd; const int* pos; int vocab /* backward only */; const float* Wp; int Fo; const float* bias; float drop_p;
    const unsigned* mask; const float *norm, *pw; float *coef, *wsum; int* gid; float *Z, *hg; long long ld_hg;   /* hg NULL: forward stops at Z */
};
struct txe_gcn_fold_grads { float *dW, *d_b, *dP, *d_pw; };
int txe_gcn_collapse_fwd(const struct txe_graph_batch* batch, const struct txe_gcn_fold_layer* layer, void* ws, size_t ws_bytes, void* stream);
int txe_gcn_collapse_bwd(const struct txe_graph_batch* batch, const struct txe_gcn_fold_layer* layer, const float* d_hg, long long ld_dhg,
                         int act_on, float act_slope, float* d_X, const struct txe_gcn_fold_grads* grads,
                         int dz_given /* d_hg IS dZ [G][Kp]: no product, dW / d_b not written (txe_bilinear_folded_*, wf_by_k) */, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- egonet construction + batching on device: data_loader/dataset.py:404-437 (_get_subgraph) + dgl.batch (data_loaders.py:25).
 * Taxonomy as parent CSR (par_ptr/par_idx) and child CSR (chd_ptr/chd_idx); anchors [G]; exclude [G] or NULL (query node removed
 * from each egonet's siblings, -1 = none: the positive example of dataset.py:421-424); children beyond `expand` are drawn with
 * replacement from a counter-based hash of (seed, index_base + egonet, draw) -- index_base = position of the batch's first egonet in the
 * caller's whole list, so that a list cut into `-b` chunks (test_fast.py:149-179) draws what the single batch draws.  Step 1 gives node_off [G+1] (node_off[G] = N; E = 2N - G), step 2
 * the node table (ids, pos [N]) and both CSR views in closed form (no sort). */
size_t txe_egonet_ws_bytes(int G);
int txe_egonet_offsets(const int* par_ptr, const int* chd_ptr, const int* chd_idx, const int* anchors, const int* exclude, int G,
                       int expand, unsigned long long seed, int index_base, int* node_off, void* ws, size_t ws_bytes, void* stream);
int txe_egonet_fill(const int* par_ptr, const int* par_idx, const int* chd_ptr, const int* chd_idx, const int* anchors,
                    const int* exclude, int G, int expand, unsigned long long seed, int index_base, const int* node_off, int* ids, int* pos,
                    int* rowptr_in, int* col_src, int* eid_in, int* rowptr_out, int* col_dst, int* pos_out, void* stream);

/* ---- the samplers' arguments, grouped by what they are (txe_sample_anchors and txe_sample_groups read the first two): plain structs of
 * borrowed device pointers and scalars; the caller keeps what they point to alive and may fill `source` once for all its launches. */
struct txe_sample_source {     /* the resident arrays: node_list, the query-parent CSR (n_par_idx: the length of par_idx), the mask CSR (rows
                                * sorted), the negative pool (ascending; n_pool entries) and k = negative_size */
    const int *node_list, *par_ptr, *par_idx; int n_par_idx; const int *mask_ptr, *mask_idx, *pool; int n_pool, k;
};
struct txe_sample_span {       /* which queries -- positions start .. start+Q-1 of the epoch order (order [n_order]: indices into node_list) --
                                * and the hash's inputs; repeated != 0: the run layout */
    const int* order; int n_order, start, Q, epoch; unsigned long long seed; int repeated;
};
struct txe_sample_hard {       /* the mined table: idx [n_queries, H] int32, row i for node_list[i], node ids best first; cnt [n_queries] the
                                * valid entries of each row; slots: the first negative slots of a query that come from its row */
    const int *idx, *cnt; int H, slots;
};
struct txe_sample_near {       /* the MASKED taxonomy's parent and child CSR over n_nodes nodes (n_par / n_chd: the lengths of par_idx / chd_idx;
                                * not the source's query-parent CSR), the sibling / grandparent / uncle slot counts, and counts [3] += the
                                * accepted proposals of each class */
    const int *par_ptr, *par_idx, *chd_ptr, *chd_idx; int n_nodes, n_par, n_chd, n_sib, n_gpar, n_unc; int* counts;
};

/* ---- training-anchor sampling on device, sampling_mode 1: data_loader/dataset.py:334-381 (one positive through the positive pointer,
 * exactly k negatives) for the span's Q queries.  One launch of ONE kernel body, compiled three times; which one runs is decided by the
 * pointers, not by the counts: near != NULL: near + optional table + pool (hard may be NULL: no table slots); else hard != NULL: table +
 * pool; else the pool alone.  A slot no rule below claims, or whose proposal a rule refuses, is the same code in all three -- so a near
 * launch with all counts 0 writes the table launch's bytes, and a table launch with slots = 0 or an all-empty table the pool launch's.
 * Writes the index arrays of txe_egonet_offsets / txe_egonet_fill, B = Q (1 + k), packed [4B + 1]:
 *   [0, B) anchors (query i: its positive, then its k negatives) | [B, 2B) exclude (the query for the positive, -1 for negatives) |
 *   repeated == 0: [2B, 3B) the query id of every pair;  repeated != 0: [2B, 2B+Q) the distinct query ids, [3B, 3B+Q+1) run offsets i (1+k).
 * Positive: p = par_idx[par_ptr[q] + pos_ptr[q]], then pos_ptr[q] = (pos_ptr[q] + 1) % (parents of q) -- in place, the host walk exactly.
 * A query-parent row that is empty, starts below 0 or ends beyond n_par_idx is not read: p = q and the pointer stays (all three
 * instantiations; on arrays from sampler.sampler_arrays every row is sound).  A query must not appear twice among launches in flight on
 * different streams (the pointer update is not atomic).
 * The rules of negative slot j of the query at epoch position s (i = order[s], q = node_list[i]), in order:
 *   1. table (hard != NULL, hard->slots > 0): c = min(max(cnt[i], 0), H), m = min(slots, c), one rotation r = (hi32(h) c) >> 32,
 *      h = mix64(seed ^ mix64(epoch << 44 | s << 20 | 16383 << 6)) (slot value 16383 is free: k < 2^14).  Slot j < m takes
 *      idx[i H + (r + j) % c] without a rejection loop (a row's entries are distinct), unless that entry is in q's mask row, negative or
 *      above pool[n_pool - 1].
 *   2. near (near != NULL): sibling slots are j in [slots, slots + n_sib) (slots = 0 without a table), grandparent slots the next n_gpar,
 *      uncle slots the next n_unc.  The lists of the positive p:  S = chd(p);  G = par(p);  U = chd(g_0) ++ chd(g_1) ++ .. over g_i in
 *      par(p), in order (repeats stay).  Class X (list length n_X, c_X slots, t_S, t_G, t_U = 1, 2, 3) has m_X = min(c_X, n_X) and one
 *      rotation r_X = (hi32(h) n_X) >> 32, h = mix64(seed ^ mix64(epoch << 44 | s << 20 | 16383 << 6 | t_X)); the slot at class offset
 *      e < m_X proposes L_X[(r_X + e) % n_X] (an uncle index walks par(p), subtracting child counts).  A proposal is kept iff it lies in
 *      [0, n_nodes), is a pool node (binary search) and is not in q's mask row; counts[X] += the kept ones.  No rejection loop.  A row of
 *      the taxonomy CSR whose node is outside [0, n_nodes), whose start is negative, whose end lies before its start or beyond its index
 *      array counts as empty.
 *   3. pool (every other slot, and every refused proposal): attempt t = 0 .. 63 draws pool[(hi32(h) n_pool) >> 32], h = mix64(seed ^
 *      mix64(epoch << 44 | s << 20 | j << 6 | t)) (csrc/txe_common.h), accepted when not in q's sorted mask row
 *      mask_idx[mask_ptr[q] .. mask_ptr[q+1]); after 64 rejections the last draw stays and *n_padded is incremented (dataset.py:370-375
 *      pads with nodes that may be masked).
 * So no table and no taxonomy array can put an invalid or masked id into a batch.  Mined and near negatives are plain negatives (exclude
 * -1): the query can be in an anchor's egonet only when the anchor is the query, a parent or a child of it, and all of those are masked.
 * TXE_ERR_ARG (before any device work): a NULL src, span or pointer in them, a NULL pos_ptr, packed or n_padded, k < 1 or k >= 2^14, Q < 0,
 * n_pool < 1, n_par_idx < 0, n_order < 0, start < 0, start + Q > n_order or > 2^24, epoch outside [0, 2^20), 4B + 1 >= 2^31; with hard: a
 * NULL idx or cnt, H < 1, slots outside [0, k]; with near: a NULL array or counts, n_nodes < 1, a negative length or count,
 * slots + n_sib + n_gpar + n_unc > k.  The arguments are checked in order: span is not read unless src is sound.  Q == 0 with sound
 * arguments: TXE_OK, no launch. */
int txe_sample_anchors(const struct txe_sample_source* src, const struct txe_sample_span* span, int* pos_ptr, int* packed, int* n_padded,
                       const struct txe_sample_hard* hard /* NULL: no table */, const struct txe_sample_near* near /* NULL: no near slots */,
                       void* stream);

/* ---- validation-anchor sampling on device, sampling_mode 0: data_loader/dataset.py:304-307,340-355 (every parent, then at most k
 * negatives) for the Q queries at positions start .. start+Q-1 of the epoch order.  Query i's run: node2parents[q] in order (label 1,
 * exclude q), then the surviving negatives in slot order (label 0, exclude -1).  Negative slot j of epoch position s in round t draws
 * pool[(hi32(h) n_pool) >> 32], h = mix64(seed ^ mix64(epoch << 44 | s << 20 | j << 6 | t)) (as txe_sample_anchors); the query keeps the
 * unmasked draws of the first round t in 0 .. 63 that has one.  If no round has one, it keeps slot 0 of round 63 (masked) and
 * *n_padded is incremented: every query keeps 1 .. k negatives.  The batch total B = sum of the runs is known on the device only:
 * *total = B, packed [4B + 1] is laid out as txe_sample_anchors' (repeated: [3B, 3B+Q+1) the run offsets), labels [B] int64.
 * cap: the caller's capacity, >= sum of |parents| + Q k (packed holds 4 cap + 1 ints, labels cap); a B above it writes nothing but
 * *total.  ws: 3Q + 1 ints of scratch.  Three launches (count, scan, fill) on `stream`.
 * TXE_ERR_ARG (before any device work): what txe_sample_anchors refuses in src and span (one check serves both), a NULL packed, labels,
 * total, ws or n_padded, cap < Q, 4 cap + 1 >= 2^31. */
int txe_sample_groups(const struct txe_sample_source* src, const struct txe_sample_span* span, int cap, int* packed, long long* labels,
                      int* total, int* ws, int* n_padded, void* stream);

/* ---- grouped ranking of a labelled batch: model/metric.py:33-60 (obtain_ranks) on the device.  score [B] fp32, labels [B] int32
 * (label_bytes 4) or int64 (8).  Groups start at 0 and at every 0 -> 1 label transition; the rank of a positive (label 1) is 1 + the
 * negatives (label != 1) of its group strictly better in fp32 (mode 0: smaller, 1: larger; NaN and ties never count; a group without
 * negatives gives rank 1).  Writes ranks [n_pos], pos_off [n_groups + 1] (capacities B and B + 1) and counts [2] = {n_groups, n_pos};
 * nothing is read back.  TXE_ERR_ARG: a NULL pointer, B < 1, label_bytes not 4 or 8, mode not 0 or 1; TXE_ERR_WORKSPACE: ws_bytes below
 * txe_group_rank_ws_bytes(B). */
size_t txe_group_rank_ws_bytes(int B);
int txe_group_rank(const float* score, const void* labels, int label_bytes, int B, int mode, int* ranks, int* pos_off, int* counts, void* ws,
                   size_t ws_bytes, void* stream);
/* the metrics of one txe_group_rank result (model/metric.py:62-96), added in one launch to acc [n_which + 2] fp64: acc[m] += metric
 * (which >> 4m) & 15 for m < n_which (0 macro_mr, 1 micro_mr, 2 hit_at_1, 3 hit_at_3, 4 hit_at_5, 5 mrr_scaled_10, 6 combined_metrics),
 * acc[n_which] += n_groups, acc[n_which + 1] += n_pos.  TXE_ERR_ARG: a NULL pointer, n_which outside [1, 16], an id above 6. */
int txe_group_metrics(const int* ranks, const int* pos_off, const int* counts, unsigned long long which, int n_which, double* acc, void* stream);

/* ---- taxonomy-aware evaluation (taxoexpan_amd/taxometric.py): Wu & Palmer inputs and error relations of predicted parents,
 * one launch.  The taxonomy index of n_nodes nodes, built and validated on the host and trusted here: depth [n_nodes] = 1 for a node
 * without parents, else 1 + the maximum depth of its parents; anc_ptr [n_nodes + 1] / anc_idx = per node the node itself and everything
 * reachable upward, ascending by id; par_ptr [n_nodes + 1] / par_idx = the direct parents.  lca_depth(a, b) = the maximum depth over
 * anc(a) & anc(b), 0 when they share nothing.  For slot (q, r), q < Q, r < K: a = pred[q K + r], the golds of q are
 * gold_idx[gold_off[q] .. gold_off[q + 1]) (offsets clamped to [0, n_gold]; a gold outside [0, n_nodes) is skipped).  Among them j* =
 * the one with the largest 2 lca_depth(a, g_j) / (depth a + depth g_j), compared exactly as 64-bit cross products; ties by the smaller
 * relation code, then the smaller j.  Written per slot: lca_depth, best_gold = j* (the position in q's list) and relation of a to that
 * gold, the first that holds of 0 EXACT a == b, 1 ANCESTOR a in anc(b), 2 DESCENDANT b in anc(a), 3 SIBLING a direct parent in common,
 * 4 RELATED lca_depth > 0, 5 UNRELATED.  a outside [0, n_nodes) or no usable gold: lca_depth 0, best_gold -1, relation 6 (NONE).  No id
 * of pred or gold_idx is used as an address before it is compared with n_nodes.  Every output element has one writer; no atomics, no
 * floating point: the same inputs give the same bits.
 * TXE_ERR_ARG (before any launch): a NULL pointer, K < 1, Q < 0, n_nodes < 0, n_gold < 0, Q K >= 2^31.  Q == 0: TXE_OK, no launch. */
int txe_taxo_slots(const int* anc_ptr, const int* anc_idx, const int* depth, const int* par_ptr, const int* par_idx, int n_nodes,
                   const int* pred, int Q, int K, const int* gold_off, const int* gold_idx, int n_gold, int* lca_depth, int* best_gold,
                   int* relation, void* stream);

/* ---- hedged placement (taxoexpan_amd/hedge.py, csrc/txe_hedge.hip): the probability mass of every candidate's subtree
 * and the deepest candidate whose subtree mass reaches a threshold.  Everything is in candidate-column space: G candidates, column a.
 * The index, built and validated on the host (HedgeIndex.build): sub_ptr [G + 1] / sub_idx [nnz] = per column a the columns of a and
 * of all its descendants on the taxonomy, ascending, a included, each once; depth [G] = the longest-chain depth of the column's node
 * (>= 1).  The work list: item i < n_items is (item_row[i], item_slice[i], item_part[i]) -- slice s of row a covers the entries
 * sub_ptr[a] + s TXE_HEDGE_SLICE .. + TXE_HEDGE_SLICE (cut at the row's end); item_part = -1 for a row of at most TXE_HEDGE_SLICE
 * entries (one item, finished where it is summed), else the slice's position in the partial-sum workspace; long_row [n_long] = the
 * longer rows and long_ptr [n_long + 1] their ranges of workspace positions (n_part in all), in slice order.
 *
 * txe_hedge_probs: S [nq][ldS] fp32 scores, lse [nq] float64 (txe_*_score_moments_block's value at this beta), z = S or -S (negate != 0),
 * t = fl32(beta z), p = fl32(exp(float64(t) - lse[q])), and p = 0 on every row whose lse is not finite.  Written candidate-major:
 * PT[g ldq + q], ldq >= nq; the columns nq .. ldq of every row are written as zeros.  One launch; the transposition goes through a
 * padded LDS tile.  TXE_ERR_ARG before any launch: nq < 0, G < 0, beta not finite or <= 0, and (with nq > 0 and G > 0) a NULL pointer,
 * ldS < G, ldq < nq, more than 65,535 x 64 query columns.  nq == 0 or G == 0: TXE_OK, no device call.
 *
 * txe_hedge_sweep: mass[a][q] = the sum of PT[d ldq + q] over the entries d of row a, in float64, in an order fixed by the list alone:
 * every slice is summed left to right from 0.0, the slice sums are added left to right.  No atomics: equal inputs give equal bytes,
 * and a query's values do not depend on nq or on where the query sits.  n_thr == 0 (store mode): mass [G][ldm] is written, ldm >= nq.
 * 1 <= n_thr <= TXE_HEDGE_MAX_THRESHOLDS (hedge mode; thresholds: n_thr doubles in HOST memory, each in (0, 1]): per query q and
 * threshold t the column a with mass[a][q] >= thresholds[t] of the largest depth -- ties: the larger mass, then the smaller column --
 * to out_col[q n_thr + t] (int, -1 when none qualifies), with its mass to out_mass (float64, NaN for -1) and its depth to out_depth
 * (int, 0 for -1); no mass matrix is written and `mass` may be NULL.  The result for a threshold does not depend on the others.
 * Launches: the sweep (a wave per work item and tile of 64 queries), the long rows' slice sums if n_long > 0, and in hedge mode the
 * per-query merge of the workgroups' partial keys.  Every row, entry, workspace position and offset is range-checked before it
 * addresses anything; an entry outside [0, G) contributes nothing.
 * ws: txe_hedge_sweep_ws_bytes(n_items, n_long, n_part, nq, n_thr) bytes, else TXE_ERR_WORKSPACE (before any launch).
 * TXE_ERR_ARG before any launch: a negative count, n_thr > TXE_HEDGE_MAX_THRESHOLDS, a NULL thresholds with n_thr > 0, a threshold that
 * is NaN or outside (0, 1]; and (with nq > 0 and G > 0) a NULL index / work-list pointer or PT, ldq < nq, store mode with a NULL mass
 * or ldm < nq, hedge mode with a NULL output, more than 65,535 query tiles.  nq == 0 or G == 0: TXE_OK, no device call. */
#define TXE_HEDGE_SLICE 256
#define TXE_HEDGE_MAX_THRESHOLDS 8
int txe_hedge_probs(const float* S, long long ldS, int nq, int G, const double* lse, float beta, int negate, float* PT, long long ldq,
                    void* stream);
size_t txe_hedge_sweep_ws_bytes(int n_items, int n_long, int n_part, int nq, int n_thr);
int txe_hedge_sweep(const int* sub_ptr, const int* sub_idx, const int* depth, int G, int nnz, const int* item_row, const int* item_slice,
                    const int* item_part, int n_items, const int* long_row, const int* long_ptr, int n_long, int n_part, const float* PT,
                    long long ldq, int nq, const double* thresholds, int n_thr, double* mass, long long ldm, int* out_col,
                    double* out_mass, int* out_depth, void* ws, size_t ws_bytes, void* stream);

/* ---- optional per-kernel timing (debug / bench): HIP events on the launch stream around every kernel launch, with the
 * algorithmic work (flops or compulsory bytes) its launcher attributes to it.  Global state (see the conventions at the top); off by
 * default.  txe_profile_get synchronises on record i's events. */
int txe_profile_enable(int on);
int txe_profile_reset(void);
int txe_profile_count(void);
int txe_profile_get(int i, char* name_buf, int buf_len, float* ms, double* work, int* kind);
int txe_profile_stream(int i, void** stream);   /* the hipStream_t record i was launched on */

/* Order two streams of the SAME device: work submitted to `then` after this call starts only when everything submitted to `first`
 * before it has completed (an event without the system-scope fence: no L2 write-back / invalidate in front of `first`'s next kernel).
 * The host-side mirror uses it for every second-stream overlap (taxoexpan_amd/ops.py _order). */
int txe_stream_order(void* first, void* then);
/* device-to-device streaming copy with 16-byte loads / stores (n_bytes % 16 == 0, 16-byte aligned): the copy ceiling bench.py shows the
 * HBM-bound sweeps against, beside the 8 TB/s spec */
int txe_copy_stream(const void* src, void* dst, long long n_bytes, void* stream);

/* model/loss.py:52-57 info_nce_loss = F.cross_entropy(output [B][C], target [B], reduction="sum") on the [queries][1 + negatives]
 * regrouping of trainer.py:52-56, together with its gradient:  loss[0] = sum_b (logsumexp(x_b) - x_b[target_b]),
 * d_x[b][c] = softmax(x_b)[c] - [c == target_b].  target NULL = all zeros (what trainer.py:53 passes). */
int txe_info_nce(const float* x, long long ld_x, int B, int Cc, const long long* target, float* loss, float* d_x, long long ld_dx,
                 void* stream);

/* Taxonomy-aware InfoNCE (csrc/txe_taxoloss.hip): txe_info_nce with a Wu & Palmer margin on every negative.  Q groups of
 * C = 1 + k columns; x[i][c] the model's output, a[i][c] = anchors[i ld_a + c] the taxonomy node of the column's egonet, column 0 the
 * positive, p_i = a[i][0]; the index (anc_ptr, anc_idx, depth, n_nodes) and lca_depth as for txe_taxo_slots.
 *   d[i][0] = 0
 *   d[i][c] = 0                                                                     if a[i][c] or p_i lies outside [0, n_nodes)
 *                                                                                   (compared BEFORE it addresses anything)
 *   d[i][c] = 1.0 - 2.0 * lca_depth(a[i][c], p_i) / (depth[a[i][c]] + depth[p_i])   float64; in [0, 1]; 0 iff a[i][c] == p_i; 1 in a forest
 *   m[i][c] = (float)((double)gamma * d[i][c])                                      one rounding to fp32
 *   y[i][c] = x[i][c] + m[i][c]                                                     one fp32 add
 *   row_i   = logsumexp_c y[i][c] - x[i][0]
 *   loss[0] = sum_i row_i                          (row losses merged in a fixed order, in float64, then one rounding)
 *   d_x[i][c] = softmax_c(y[i])[c] - [c == 0]      (d is a constant of the batch: no gradient flows into it)
 * gamma = 0: d_x has the bytes txe_info_nce leaves on the same x with target NULL (both kernels call one row function).  margin (NULL:
 * not wanted) gets m, [Q][C] with pitch C, bit-equal to the numpy restatement loss.host_taxo_margins; dist_total (NULL: not wanted)
 * gains sum over i and c >= 1 of floor(d[i][c] 2^20), an integer atomic.  A positive whose closure row has more than
 * TXE_TAXO_STAGE_CAP entries is searched in global memory instead of LDS; the results do not depend on the route.  One launch over
 * ceil(Q / rows per workgroup) workgroups, then one launch that adds the row losses in row order: no floating-point atomics, two calls
 * on the same inputs give the same bytes in loss, d_x and margin.  After the call ws begins with the Q row losses (fp32, row order).
 * TXE_ERR_ARG before any launch: a NULL among x, anchors, anc_ptr, anc_idx, depth, loss, d_x; Q < 0, C < 1, ld_x / ld_dx / ld_a < C,
 * Q C >= 2^31, n_nodes < 0; gamma not finite or negative; ws NULL or ws_bytes < txe_info_nce_taxo_ws_bytes(Q).
 * Q == 0: TXE_OK, loss[0] = 0, nothing else written. */
#define TXE_TAXO_STAGE_CAP 64
size_t txe_info_nce_taxo_ws_bytes(int Q);
int txe_info_nce_taxo(const float* x, long long ld_x, int Q, int C, const int* anchors, long long ld_a,
                      const int* anc_ptr, const int* anc_idx, const int* depth, int n_nodes, double gamma,
                      float* loss, float* d_x, long long ld_dx,
                      float* margin /* [Q][C] pitch C, or NULL */,
                      long long* dist_total /* += sum over c >= 1 of floor(d * 2^20), or NULL */,
                      void* ws, size_t ws_bytes, void* stream);

/* In-batch negatives (csrc/txe_inbatch.hip): every query row i of S [Q][G] -- the matcher's output for (query i, egonet g) of one
 * training batch -- is a cross entropy over the batch's columns without those whose anchor lies in the query's mask row:
 *   valid(i, g) = (g == pos_col[i]) or anchor[g] not in mask_idx[mask_ptr[qnode[i]] .. mask_ptr[qnode[i] + 1])
 *   loss[0]     = sum_i (log sum_{g valid} exp S[i][g] - S[i][pos_col[i]])                 (sum-reduced, like txe_info_nce)
 *   d_out[i][g] = softmax over the valid g of row i - [g == pos_col[i]], exactly 0 where not valid; times S[i][g] under chain_exp
 *                 (S = exp(b): the gradient to b);   n_valid[i] = the valid columns of row i (>= 1: the positive)
 * mask_ptr / mask_idx: a CSR over nodes, every row ascending (sampler.sampler_arrays); both NULL: nothing is masked.  A masked column's
 * score is never used (NaN and Inf included); a NaN in a valid column makes the loss NaN.  0 <= pos_col[i] < G and
 * 0 <= qnode[i] < (nodes of the CSR) are the caller's contract.  d_out may be S itself.  One workgroup per row, then one launch that
 * adds the row losses in a fixed order in float64: no floating-point atomics, two calls on the same inputs give the same bytes
 * (valid_total is an integer atomic).  TXE_ERR_ARG before any launch: Q < 0, G < 1, Q * G >= 2^31, ld_s / ld_d < G, a NULL among S,
 * pos_col, anchor, qnode, loss, d_out, exactly one mask pointer NULL, ws NULL or ws_bytes < txe_inbatch_nce_ws_bytes(Q).
 * Q == 0: TXE_OK, loss[0] = 0, nothing else written.  After the call ws begins with the Q row losses (fp32, row order). */
size_t txe_inbatch_nce_ws_bytes(int Q);
int txe_inbatch_nce(const float* S, long long ld_s, int Q, int G, const int* pos_col, const int* anchor, const int* qnode,
                    const int* mask_ptr, const int* mask_idx,      /* both NULL: nothing is masked */
                    int chain_exp,                                  /* 1: d_out = dS * S -- the gradient to b under LBM's exp */
                    float* loss, float* d_out, long long ld_d,      /* d_out may alias S (in place) */
                    int* n_valid /* [Q] or NULL */, long long* valid_total /* += sum n_valid, or NULL */,
                    void* ws, size_t ws_bytes, void* stream);
/* B[i][g] = exp(B[i][g]) in place over [Q][G] with pitch ld_b: LBM's scores from the bilinear form, in front of txe_inbatch_nce */
int txe_inbatch_exp(float* B, long long ld_b, int Q, int G, void* stream);

/* ---- the reference's other training losses on a labelled score vector (csrc/txe_pairloss.hip): x [B] fp32, labels [B] int32
 * (label_bytes 4) or int64 (8), read as they are.  An entry is a POSITIVE iff its label is 1.  Each call leaves the sum-reduced loss in
 * loss[0] and its gradient in d_x [B]; no host synchronisation, no floating-point atomics: two calls on the same input give the same
 * bits.  TXE_ERR_ARG (before any device work, nothing written): a NULL pointer, B < 1, label_bytes not 4 or 8, a non-finite beta /
 * margin; TXE_ERR_WORKSPACE: ws_bytes below txe_margin_rank_loss_ws_bytes(B).
 *
 * model/loss.py:21-29 bce_loss = F.binary_cross_entropy_with_logits(output.squeeze(), 1.0 - target.float(), reduction="sum") (the target
 * is inverted: the score is an energy, loss.py:26):  loss = sum over positives of softplus(x_i) + sum over every other entry of
 * softplus(-x_i), softplus(z) = max(z, 0) + log1p(exp(-|z|)) (finite for x = +-1e4);  d_x[i] = sigmoid(x_i) - [i is no positive].
 * The contract is labels in {0, 1}.  One launch. */
int txe_bce_loss(const float* x, const void* labels, int label_bytes, int B, float* loss, float* d_x, void* stream);
/* model/loss.py:12-19 square_exp_loss = (output[target==1]**2).sum() + beta * torch.exp(-1.0*output[target==0]).sum():
 * loss = sum over positives of x_i^2 + beta * sum over label == 0 EXACTLY of exp(-x_i) (any other label contributes nothing);
 * d_x[i] = 2 x_i for a positive, -beta exp(-x_i) for label 0, else 0.  exp overflows to +Inf / -Inf in fp32 as torch's does.
 * One launch. */
int txe_square_exp_loss(const float* x, const void* labels, int label_bytes, int B, float beta, float* loss, float* d_x, void* stream);
/* model/loss.py:31-50 margin_rank_loss (label.cpu(), a regex over the label bytes, itertools.product, then
 * F.margin_ranking_loss(pos, neg, -1, margin, reduction="sum")) without the read-back.  Groups start at index 0 and at every i with
 * label[i-1] == 0 and label[i] == 1 (txe_group_rank's rule); within a group every (positive p, negative n) pair -- a negative is every
 * entry that is no positive -- contributes max(0, (x_p - x_n) + margin), the condition evaluated in fp32 exactly as written (one
 * subtraction, one addition).  d_x[p] = +(negatives of its group with (x_p - x_n) + margin > 0), d_x[n] = -(positives of its group with
 * the same): integer-valued, bit-equal to torch autograd's.  NaN never compares true (no gradient; the loss is NaN, as torch's clamp
 * gives); a group without negatives or without positives contributes nothing.  On label vectors whose every group is >= 1 ones followed
 * by >= 1 zeros this is the reference's pair list; on a vector that begins with a zero the reference's bookkeeping drops the pairs
 * (loss 0) and this follows the group rule.  Five enqueued steps on `stream` (flags, one 64-bit scan, index, pairs, finish): positives'
 * counts are added with integer atomics, per-tile loss partials are combined in a fixed order.  ws is sized from B alone. */
size_t txe_margin_rank_loss_ws_bytes(int B);
int txe_margin_rank_loss(const float* x, const void* labels, int label_bytes, int B, float margin, float* loss, float* d_x, void* ws,
                         size_t ws_bytes, void* stream);

/* trainer.py:61 `self.optimizer.step()` for torch.optim.Adam (config.mag.json:66-73: lr 1e-3, weight_decay 0, amsgrad true): the whole
 * parameter set in one launch.  params / grads / exp_avg / exp_avg_sq / max_exp_avg_sq are HOST arrays of n_tensors DEVICE pointers
 * (dense fp32, numel[t] elements); max_exp_avg_sq == NULL selects plain Adam; `step` >= 1 is the count of this update.
 *   g' = g + weight_decay p;  m = lerp(m, g', 1-beta1);  v = beta2 v + (1-beta2) g'^2;  vmax = max(vmax, v)
 *   p -= lr / (1-beta1^step) * m / (sqrt(vmax) / sqrt(1-beta2^step) + eps) */
int txe_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  float* const* max_exp_avg_sq, const long long* numel, double lr, double beta1, double beta2, double eps,
                  double weight_decay, long long step, void* stream);

/* txe_adam_step behind a guard: two DEVICE scalars that the launches of this step read once per workgroup, before any per-element
 * work, and never write.  Either may be NULL; both NULL is txe_adam_step itself (the same launches, the same bits).
 *   first_bad   *first_bad >= 0: every workgroup returns before its first load -- params, exp_avg, exp_avg_sq and max_exp_avg_sq are
 *               left untouched.  The host still counts the step; optim.Adam.discount_frozen_steps takes such steps back.
 *   gnorm2      the squared global L2 norm of the gradients.  coef64 = max_grad_norm / (sqrt(*gnorm2) + 1e-6) in fp64
 *               (torch.nn.utils.clip_grad_norm_'s formula), coef = coef64 < 1 ? (float)coef64 : 1, and every gradient element is
 *               multiplied by coef before the weight-decay term (g * 1.0f is g: an inactive clip changes no bit).  `grads` are not
 *               written.  max_grad_norm is ignored when gnorm2 is NULL; otherwise it must be finite and > 0 (TXE_ERR_ARG, nothing
 *               launched).  A *gnorm2 that is not finite, met without a first_bad pointer, goes through the formula as written: NaN
 *               gives coef 1, +Inf gives coef 0 (and NaN in the elements that are Inf); no parity with torch is claimed for that case.
 * ORDERING CONTRACT: both scalars must have been written by work enqueued EARLIER ON THE SAME `stream` (txe_step_log's first_bad word
 * and its gnorm2_log[step] slot are; every launch of one step reads the same two values).  A value written from another stream or by
 * the host without an ordering against `stream` may or may not be seen. */
int txe_adam_step_guarded(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const long long* numel, double lr, double beta1,
                          double beta2, double eps, double weight_decay, long long step, const double* gnorm2,
                          const long long* first_bad, double max_grad_norm, void* stream);

/* txe_adam_step_guarded with an exponential moving average of the parameters formed in the same launches (an addition: the reference has
 * no weight averaging).  ema is a seventh HOST array of n_tensors DEVICE pointers (dense fp32, numel[t] elements, no overlap with any
 * other buffer).  After the update of an element the same thread forms, in fp32,
 *   e = fma(one_minus_d, p_new - e, e),   one_minus_d = (float)(1.0 - ema_decay),   p_new = the parameter value this step stores
 * -- lerp(e, p_new, 1 - ema_decay) in the form exp_avg uses.  ema_decay is the effective decay of THIS step (a warm-up schedule is the
 * host's: optim.ema_decay_at); it must satisfy 0 <= ema_decay < 1, else TXE_ERR_ARG with nothing launched -- this check comes before every
 * other one.  A NULL ema[t] of a non-empty tensor is TXE_ERR_ARG.  The update itself does not depend on e: params, exp_avg, exp_avg_sq and
 * max_exp_avg_sq get the bits txe_adam_step_guarded gives them.  An active clip changes g, hence p_new, hence e; a frozen step
 * (*first_bad >= 0) returns before any load and leaves e untouched as well.  e is read and written with the accesses of the other
 * buffers: 16 bytes per thread where all seven pointers of a tensor are 16-byte aligned, element by element otherwise.
 * ema == NULL: txe_adam_step_guarded itself -- the same launches, the same bits; ema_decay is ignored.
 * gnorm2 / first_bad / max_grad_norm keep the meaning and the ORDERING CONTRACT of txe_adam_step_guarded. */
int txe_adam_step_ema(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      float* const* max_exp_avg_sq, float* const* ema, const long long* numel, double lr, double beta1, double beta2,
                      double eps, double weight_decay, long long step, double ema_decay, const double* gnorm2,
                      const long long* first_bad, double max_grad_norm, void* stream);

/* a[t][i] <-> b[t][i] for n_tensors pairs of dense tensors of numel[t] 32-bit elements (HOST arrays of DEVICE pointers), up to 24 pairs
 * per launch.  The exchange moves 32-bit words, never floats: NaN payloads, -0.0 and denormals arrive bit for bit; two calls restore both
 * sides.  Empty pairs are skipped.  TXE_ERR_ARG (nothing launched): n_tensors < 0, a NULL table with n_tensors > 0, a negative numel, a
 * NULL pointer of a non-empty pair.  OVERLAP IS NOT SUPPORTED: the two tensors of a pair, and the tensors of different pairs, must not
 * share memory (every element is read and written by one thread, with no ordering between threads). */
int txe_tensor_swap(int n_tensors, float* const* a, float* const* b, const long long* numel, void* stream);

/* The per-step device log of the training loop (what trainer.py:63-65 reads back with `loss.item()` every step; csrc/txe_steplog.hip):
 * one call per step, enqueued between `loss.backward()` and `optimizer.step()`; nothing returns to the host.
 *   loss_log[step]   = loss[0]                                     (fp32 device scalar)
 *   gnorm2_log[step] = sum over every element g of every gradient tensor of (double)g * (double)g
 *   acc[0] += (double)loss[0];  acc[1] += 1                        (the epoch's loss sum and its number of logged steps)
 *   first_bad[0] = step  if first_bad[0] < 0 and loss[0] or any gradient element is not finite  (the owner initialises it to -1)
 * grads is a HOST array of n_tensors DEVICE pointers (dense fp32, numel[t] elements; an empty tensor is skipped; n_tensors == 0 logs the
 * loss alone); the table travels in the kernel argument.  Every workgroup squares and sums one run of TXE_STEP_LOG_CHUNK consecutive
 * elements of one tensor in fp64 and stores its partial in ws; the workgroup that draws the last ticket of an integer counter adds the
 * partials in a fixed order (no floating-point atomics anywhere): the logged value is a pure function of the gradients, bit-identical
 * from run to run.  That workgroup also updates acc and first_bad with plain read-modify-writes: the calls of one log must be ordered
 * on one stream.
 * ws: txe_step_log_ws_bytes(n_chunks) bytes, n_chunks = sum over the tensors of ceil(numel[t] / TXE_STEP_LOG_CHUNK), 16-byte aligned;
 * its first 16 bytes (the ticket) are ZEROED ONCE by the owner before the first call and left zero by every call.
 * TXE_ERR_ARG (nothing launched): a NULL loss / log pointer / ws, step outside [0, capacity), n_tensors < 0, a NULL table with
 * n_tensors > 0, a negative numel or a NULL pointer of a non-empty tensor; TXE_ERR_WORKSPACE: ws_bytes too small. */
#define TXE_STEP_LOG_CHUNK 4096
size_t txe_step_log_ws_bytes(int n_chunks);
int txe_step_log(const float* loss, int n_tensors, const float* const* grads, const long long* numel, long long step, long long capacity,
                 float* loss_log, double* gnorm2_log, double* acc, long long* first_bad, void* ws, size_t ws_bytes, void* stream);

/* ---- the term-embedding table as a trainable input (csrc/txe_rowgrad.hip; an addition: the reference freezes its embeddings).
 * A batch reads the table through two gathers -- ids_a [n_a], the batch's `_id` (x = features[_id]), and ids_b [n_b], the distinct query
 * ids -- and backward leaves one gradient row per occurrence: d_a [n_a][ld_a >= d], d_b [n_b][ld_b >= d].  Occurrence i < n_a is a's
 * i-th, occurrence n_a + j is b's j-th.  Either side may be empty.
 *
 * txe_rowgrad_group sorts the occurrences by table row -- one STABLE radix sort over the ceil(log2(n_rows + 1)) key bits, so within a
 * row the occurrence indices ascend, all of a's before b's -- and lists the segments.  An id outside [0, n_rows) is given the key n_rows
 * before anything is addressed with it: it forms the last segment, which nothing reads; it is never an error.  ws afterwards, as int32
 * words, e = the smallest multiple of 64 >= max(n_a + n_b, 1):
 *   [0]                    n_seg, the number of segments (the dropped ids' segment included)
 *   [64, 64 + n)           rows: the sorted keys              [64 + e, ...)   occ: the occurrence indices in sorted order
 *   [64 + 2e, ... + n_seg) heads: the sorted position at which segment s begins (ascending; segment s ends where s + 1 begins, the last at n)
 * and scratch behind.  n_a + n_b == 0: TXE_OK, nothing launched, ws not looked at.
 *
 * txe_sparse_adam_rows: for every row that occurs (and whose trainable byte, if the array is given, is not 0) the gradient rows of its
 * occurrences are summed in fp32 in an order that depends on the segment's length L alone,
 *   L <= 64:  s = g_0; s = s + g_k (k = 1 .. L-1)
 *   L >  64:  c = ceil(L / 16); the slices [j c, min(L, (j+1) c)) are summed as above into p_j; s = p_0; s = s + p_j (j = 1 .. ceil(L / c) - 1)
 * and txe_adam_step's update with weight_decay 0 and `step` (the GLOBAL count of this update, >= 1) is applied to that row of weight,
 * exp_avg, exp_avg_sq and max_exp_avg_sq (NULL: plain Adam), all [n_rows][ld_w >= d]: the same expression with the same fma placement,
 * element for element.  Rows that do not occur are neither read nor written (lazy Adam: their moments do not decay); there is no
 * weight_decay argument because a decay applied only to the rows of a batch would be another regulariser than the dense one.  One
 * writer per table element, no floating-point atomics: two calls on the same inputs give the same bytes.  ws is what txe_rowgrad_group
 * left for the same ids, n_a, n_b and n_rows, enqueued earlier on the same stream.  first_bad has the meaning and the ORDERING CONTRACT
 * of txe_adam_step_guarded: *first_bad >= 0 and no thread loads or stores anything.  Accesses are 16 bytes per lane where every pointer
 * is 16-byte aligned and every pitch a multiple of 4, 8 bytes where 8 and 2 hold, single elements otherwise.
 * TXE_ERR_ARG with nothing launched (both entry points, as far as they have the argument): a negative count, n_a + n_b >= 2^31, d < 1,
 * a NULL ids / gradient pointer of a non-empty side, a pitch below d, a NULL weight / exp_avg / exp_avg_sq, step < 1, a beta outside
 * [0, 1), and with n_a + n_b > 0 a NULL ws or ws_bytes < txe_rowgrad_ws_bytes(n_a, n_b).  The scratch part of that size is asked of the
 * sort and select library once per n; a query that fails makes txe_rowgrad_ws_bytes 0 and the two entry points TXE_ERR_LAUNCH (on a host
 * without a GPU, where nothing can be launched and only these checks run, the scratch counts as 0: a size holds for the machine it was
 * asked on). */
/* txe_rows_run_sum: the backward of ops.RepeatedRows.dense() when the distinct query rows ask for a gradient: dst [U][ld_dst >= r], row
 * u = src[run_off[u]] + src[run_off[u] + 1] + ... + src[run_off[u+1] - 1] of src [G][ld_src >= r], fp32, left to right (an empty run
 * gives 0; offsets are clamped to [0, G]) -- no atomics, the same bytes every time, where torch's index_add_ of repeat_interleave's
 * backward promises no order.  TXE_ERR_ARG: a negative count, r < 1, a pitch below r, a NULL pointer with U > 0.  U == 0: no launch. */
int txe_rows_run_sum(const float* src, long long ld_src, const int* run_off, int U, int G, int r, float* dst, long long ld_dst, void* stream);
size_t txe_rowgrad_ws_bytes(int n_a, int n_b);
int txe_rowgrad_group(const int* ids_a, int n_a, const int* ids_b, int n_b, int n_rows, void* ws, size_t ws_bytes, void* stream);
int txe_sparse_adam_rows(float* weight, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long long ld_w, int n_rows, int d,
                         const float* d_a, long long ld_a, int n_a, const float* d_b, long long ld_b, int n_b, const void* ws,
                         size_t ws_bytes, const unsigned char* trainable, double lr, double beta1, double beta2, double eps,
                         long long step, const long long* first_bad, void* stream);

/* ---- fp32 products on the bf16 matrix pipe (replaces the fp32-MFMA route of model_zoo.py:83 `self.fc(...)` for the first
 * layer's projection).  A packed operand holds every fp32 element as the EXACT sum of three bf16 numbers (three planes, stored as 1-KB
 * MFMA fragments: csrc/txe_gemm_split.h); txe_gemm_nt_split forms C [M][N] = A [M][K] B[N][K]^T from six of the nine plane products with
 * fp32 accumulation -- the dropped terms are a quarter of an fp32 multiply's own rounding error in the root mean square (at most twice it).
 * side 0 = the operand whose rows are C's rows, side 1 = the operand whose rows are C's columns.
 * The whole fp32 domain is covered (csrc/txe_gemm_split.h): a packed fragment that holds +-Inf, NaN or |x| >= 2^120 is stored raw with a
 * NaN marker plane, the product kernels check their accumulators after the k-loop and a tile that is not finite recomputes itself with fp32
 * FMAs over the exactly decoded operands -- the same entries are NaN / +Inf / -Inf as in an IEEE fp32 product (tests/test_gpu_split_gemm.py
 * *_on_the_whole_fp32_domain), at scalar speed for those tiles only.  Nonzero |x| < 2^-100 is carried to 2^-126 ABSOLUTE (flush-to-zero
 * semantics, as GPU fp32 units treat subnormals: such elements are routine in gradients and stay on the fast path). */
size_t txe_split_packed_bytes(int rows, int cols);
int txe_split_pack(const float* src, long long ld, int rows, int cols, int side, void* packed, void* stream);   /* side 2 / 3: side 0 / 1 of
    a matrix given as its transpose, src [cols][ld >= rows] */
int txe_gemm_nt_split(const void* A_packed, const void* B_packed, int M, int N, int K, float* C, long long ldc, void* stream);

/* The TN form (weight gradients, model_zoo.py:83 backward: dW = d_Y^T X over the nodes): part[z][M][ldc] = A[rows of slice z]^T B[same rows],
 * z < S, slices of ksplit rows (a multiple of 16).  A [n_rows][lda] is fp32 (split in the product's loader), B comes packed
 * contraction-major by txe_split_pack_t (cols % 4 == 0, 16-byte aligned rows; the last 160-column tile is zero-filled).  M % 128 == 0; lda % 4 == 0, A 16-byte aligned and
 * n_rows * lda * 4 < 2^31 (32-bit byte offsets), else TXE_ERR_ARG -- txe_gat_dense_bwd falls back to the fp32 MFMA by itself. */
size_t txe_split_packed_t_bytes(int rows, int cols);
int txe_split_pack_t(const float* src, long long ld, int rows, int cols, void* packed, void* stream);
int txe_gemm_tn_split(const float* A, long long lda, int M, const void* B_packed_t, int N, int n_rows, int S, int ksplit, float* part,
                      long long ldc, long long split_stride, void* stream);

/* host-side evaluation of the counter-based dropout hash the kernels inline (uniform in [0,1)); keep = u >= p */
float txe_dropout_uniform_host(unsigned long long seed, unsigned long long idx);
unsigned txe_dropout_mask_word_host(unsigned long long seed, unsigned long long word_index, float p);

#ifdef __cplusplus
}
#endif
#endif /* TXE_H */
