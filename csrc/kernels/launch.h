// The C entry points of the gfx950 kernels: every mivc_* function a .hip file defines, declared
// once.  Plain C++ (no HIP, no pybind11): the defining .hip and the pybind11 shim
// (bindings_hip.cc) both include this header, so a definition or a call that drifts from the
// declaration fails to compile ("conflicting types") where C linkage alone would link it.
// Device pointers are typed, record arrays (MbHeader, SlotRoute, ...) cross as void*, and the
// HIP stream is a void*.
#pragma once
#include <cstddef>
#include <cstdint>

#include "geom_limits.h"
#include "hevc_decode.h"

extern "C" {
// ---- synth.hip
void mivc_launch_synth(void* y, void* u, void* v, int width, int height, int slots, int frames, int frame0,
                       uint32_t seed, int bit_depth, int slot0, void* stream, int kind);
// ---- frame_prep.hip
void mivc_launch_prep(const uint8_t* in_y, const uint8_t* in_u, const uint8_t* in_v, int w, int h,
                      int64_t in_stride_y, int64_t in_stride_c, int nframes, uint8_t* out_y, uint8_t* out_u,
                      uint8_t* out_v, int ow, int oh, int W, int H, void* stream, const int* fsel);
void mivc_launch_rgb_to_i420(const uint8_t* rgb, int w, int h, int nframes, uint8_t* y, uint8_t* u, uint8_t* v,
                             void* stream);
// ---- scale.hip
int mivc_launch_scale(const void* in, int w, int h, long long in_stride, long long in_pitch, void* out, int ow, int oh,
                      int W, int H, long long out_stride, long long out_pitch, int nframes, const int* fx,
                      const int16_t* cx, int tx, const int* fy, const int16_t* cy, int ty, int tile_w, int tile_h,
                      int in_cols, int in_rows, int bd, void* stream);
// ---- aq.hip
void mivc_launch_aq_offsets(int B, int wmb, int hmb, const uint8_t* sy, const uint8_t* su, const uint8_t* sv,
                            float strength, const float* extra, long long extra_stride, int8_t* out, void* stream,
                            const void* route);
void mivc_launch_aq_terms(int B, int wmb, int hmb, const uint8_t* sy, const uint8_t* su, const uint8_t* sv, float* terms,
                          void* stream);
void mivc_launch_aq_auto_finish(int B, int nmb, const float* terms, int mode, float strength, const float* extra,
                                long long extra_stride, int8_t* out, void* stream, const void* route);
int mivc_launch_prep_aq(const uint8_t* in_y, const uint8_t* in_u, const uint8_t* in_v, int w, int h, int64_t in_stride_y,
                        int64_t in_stride_c, int B, uint8_t* out_y, uint8_t* out_u, uint8_t* out_v, int W, int H,
                        const int* fsel, float strength, const float* extra, long long extra_stride, int8_t* out,
                        void* stream, const void* route);
int mivc_launch_prep_aq_terms(const uint8_t* in_y, const uint8_t* in_u, const uint8_t* in_v, int w, int h,
                              int64_t in_stride_y, int64_t in_stride_c, int B, uint8_t* out_y, uint8_t* out_u,
                              uint8_t* out_v, int W, int H, const int* fsel, float* terms, void* stream);
void mivc_launch_qp_fixup(int B, int wmb, int hmb, void* hdr, const int16_t* coef, const uint8_t* nz, uint8_t* flags,
                          const int* slice_qp, void* stream, int slice_rows, const uint8_t* pre, const void* route);
// ---- me.hip
void mivc_launch_me_halfpel(int B, int W, int H, const uint8_t* ref_y, uint8_t* hp, void* stream, const void* route,
                            int nbuf);
void mivc_launch_me(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref_y, const int16_t* pred_mv,
                    int16_t* out_mv, int* out_cost, uint8_t* out_pred, int* out_intra_cost, const int* qp, int range,
                    int subpel, uint8_t* hp, const int8_t* aq, int planes_ready, int early_sad, void* stream,
                    const int* gate_cost, int gate_thresh, const int16_t* cost_mv, const void* route, int nbuf,
                    int role, int want, const int16_t* seed_mv);
void mivc_launch_me_ref_select(int B, int wmb, int hmb, int nref, int16_t* mv, int16_t* mv8, int* cost, uint8_t* pred,
                               const int16_t* xmv, const int* xcost, const uint8_t* xpred, int8_t* mref, const int* qp,
                               const int8_t* aq, void* stream, const void* route);
void mivc_me_prof_read(unsigned long long* out);  // MIVC_ME_PROFILE builds only (tools/prof_me.py)
// ---- h264_p_refine.hip
void mivc_launch_p_refine(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref, const uint8_t* hp,
                          const int16_t* mv_in, int16_t* mv_out, int* cost, const int16_t* pm, uint8_t* pred,
                          const int* qp, const int8_t* aq, void* stream, const void* route, int nbuf,
                          const uint8_t* chg_in, uint8_t* chg_out);
void mivc_launch_p_part8(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref, const uint8_t* hp,
                         const int16_t* mv, const int16_t* pm, int* cost, uint8_t* pred, int16_t* mv8, const int* qp,
                         const int8_t* aq, int overhead, int min_satd, void* stream, const void* route, int nbuf,
                         const int* bits16, const uint8_t* dir16);
// ---- h264_p_mixed.hip
void mivc_launch_p_mixed_refs(int B, int wmb, int hmb, int nref, int16_t* mv, int16_t* mv8, int* cost, uint8_t* pred,
                              const int16_t* xmv, const int* xcost, const uint8_t* xpred, int8_t* mref, int8_t* mref4,
                              const int* qp, const int8_t* aq, const uint8_t* src0, const uint8_t* src,
                              const uint8_t* ref, const uint8_t* hp, const int16_t* pm, const int16_t* scale,
                              int overhead, int min_satd, void* stream, const void* route, int nbuf);
// ---- h264_b.hip
void mivc_launch_b_direct(int B, int wmb, int hmb, const void* col, const int* dsf, const int* direct_copy, int nref,
                          int16_t* dmv, int8_t* dref, int16_t* pm0, int16_t* pm1, void* stream, const void* route,
                          int nbuf, uint8_t* czero, const int8_t* cmap);
void mivc_launch_b_decide(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref0, const uint8_t* ref1,
                          const uint8_t* hp0, const uint8_t* hp1, const int16_t* mv0, const int16_t* mv1,
                          const int* cost0, const int* cost1, const uint8_t* pred0, const uint8_t* pred1,
                          const int16_t* pm0, const int16_t* pm1, const int16_t* dmv, const int* qp, const int8_t* aq,
                          void* hdr, uint8_t* pred_out, int* cost_out, void* stream, const int* w1, int nref,
                          const int8_t* dref, const uint8_t* const* ref0k, const uint8_t* const* hp0k,
                          int direct_only, int bparts, int have_direct, int spatial, int dbias, const void* route,
                          int nbuf, const uint8_t* czero);
void mivc_launch_b_spatial(int B, int wmb, int hmb, void* hdr, const void* col, const uint8_t* src, const uint8_t* ref1,
                           const uint8_t* hp1, const uint8_t* const* ref0k, const uint8_t* const* hp0k, const int* w1,
                           int nref, uint8_t* pred_out, int* err, void* stream, const int* intra_cost, int* cost,
                           const int* qp, const int8_t* aq, int bias, const void* route, int nbuf);
void mivc_launch_b_spatial_exact(int B, int wmb, int hmb, void* hdr, const int* intra_cost, const int* cost,
                                 const uint8_t* czero, uint8_t* fix, void* stream, const void* route, int slice_rows,
                                 int tol);
void mivc_launch_b_spatial_fixup(int B, int wmb, int hmb, const void* hdr, const uint8_t* fix, const uint8_t* ref0,
                                 const uint8_t* hp0, const uint8_t* ref1, const uint8_t* hp1, uint8_t* pred_out,
                                 void* stream, const void* route, int nbuf);
// ---- encode_inter.hip
void mivc_launch_encode_inter(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* src_u,
                              const uint8_t* src_v, const uint8_t* ref_y, const uint8_t* ref_u, const uint8_t* ref_v,
                              uint8_t* rec_y, uint8_t* rec_u, uint8_t* rec_v, const uint8_t* pred_y,
                              const int16_t* mv, const int* me_cost, const int* intra_cost, const int* qp,
                              int chroma_qp_offset, void* hdr, int16_t* coef, uint8_t* nz, uint8_t* intra_flag,
                              int* intra_count, const int8_t* aq, const uint8_t* ref1_u, const uint8_t* ref1_v,
                              int bmode, int t8, const int16_t* mv8, void* stream, const int* w1, int nref,
                              const uint8_t* const* xref_u, const uint8_t* const* xref_v, const int8_t* mref,
                              const int* wp, int trellis, float trellis_lambda, const void* route, int nbuf,
                              uint8_t* qp_flags, uint32_t* mask_pre, const int8_t* mref4);
// ---- encode_intra.hip
void mivc_launch_encode_intra(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* src_u,
                              const uint8_t* src_v, uint8_t* rec_y, uint8_t* rec_u, uint8_t* rec_v, const int* qp,
                              int chroma_qp_offset, void* hdr, int16_t* coef, uint8_t* nz,
                              const uint8_t* intra_flag, const int* intra_count, int* err, int use_i4x4,
                              const int8_t* aq, void* stream, int use_i8x8, const void* route, int nbuf,
                              int slice_rows, int trellis, float trellis_lambda, int* gprog, long long gprog_ints);
void mivc_intra_prof_read(unsigned long long* out);  // MIVC_INTRA_PROFILE builds only (tools/prof_intra.py)
// ---- deblock.hip
void mivc_launch_deblock_bs(int B, int wmb, int hmb, const void* hdr, const uint8_t* nz, uint8_t* bs, uint32_t* info,
                            void* stream, const void* route);
void mivc_launch_deblock(int B, int wmb, int hmb, uint8_t* rec_y, uint8_t* rec_u, uint8_t* rec_v, const uint8_t* bs,
                         const uint32_t* info, int chroma_qp_offset, int alpha_off, int beta_off, int* err,
                         void* stream, const void* route, int nbuf);
void mivc_launch_deblock_dpb(int B, int wmb, int hmb, int dpb_n, uint8_t* dpb_y, uint8_t* dpb_u, uint8_t* dpb_v,
                             const int16_t* cur_idx, const void* hdr, const uint8_t* bs, int chroma_qp_offset,
                             int alpha_off, int beta_off, int* err, void* stream);
// ---- deblock16.hip
void mivc_launch_deblock_dpb16(int B, int wmb, int hmb, int dpb_n, uint16_t* dpb_y, uint16_t* dpb_u, uint16_t* dpb_v,
                               const int16_t* cur_idx, const void* hdr, const uint8_t* bs, int chroma_qp_offset,
                               int alpha_off, int beta_off, int bd, int* err, void* stream);
// ---- decode.hip
void mivc_launch_decode_picture_dpb(int B, int wmb, int hmb, int dpb_n, uint8_t* dpb_y, uint8_t* dpb_u, uint8_t* dpb_v,
                                    const int16_t* cur_idx, const int16_t* reftab, const int16_t* wp, const int16_t* sub,
                                    const void* hdr, const uint32_t* mask, const uint32_t* off,
                                    const int16_t* coef, const int8_t* run, int any_inter, int chroma_qp_offset,
                                    uint8_t* nz, int* err, void* stream);
void mivc_launch_decode_picture_dpb16(int B, int wmb, int hmb, int dpb_n, uint16_t* dpb_y, uint16_t* dpb_u,
                                      uint16_t* dpb_v, const int16_t* cur_idx, const int16_t* reftab, const int16_t* wp,
                                      const int16_t* sub, const void* hdr, const uint32_t* mask, const uint32_t* off,
                                      const int16_t* coef, const int8_t* run, int any_inter, int chroma_qp_offset, int bd,
                                      uint8_t* nz, int* err, void* stream);
// ---- cabac.hip
size_t mivc_cabac_nb_bytes();
int mivc_cabac_gap();
int mivc_cabac_read_ahead();
void mivc_launch_cabac_bin(int B, int wmb, int hmb, const void* hdr, const int16_t* coef, uint32_t* mask, void* nb,
                           int* cnt, long long* off, int* tot, uint16_t* pool, long long pool_cap,
                           long long* pool_used, long long* base, int* total, const int* slot_qp, int slice_type,
                           int num_ref_l0, int num_ref_l1, int t8x8_mode, int* err, void* stream, const void* route,
                           int slice_rows, const uint32_t* pre);
void mivc_launch_cabac_code(int L, int B, uint16_t* pool, const long long* base, const int* total,
                            const uint32_t* hdr_bits, const int* hdr_nbits, const int* slot_qp,
                            unsigned long long itypes, int* bytes, uint8_t* out, long long* out_off, int* err,
                            uint8_t* host_out, long long host_cap, void* stream);
// ---- cavlc.hip
size_t mivc_cavlc_mb_bytes();
void mivc_launch_cavlc(int B, int wmb, int hmb, const void* hdr, const int16_t* coef, void* mbs, int* len,
                       long long* off, int* trail, long long* total_bits, int* slot_bytes, uint32_t* words,
                       long long cap_words, const uint32_t* hdr_bits, const int* hdr_nbits, int pslice, int slice_qp,
                       const int* slot_qp, uint8_t* out, long long* out_off, const uint8_t* nz, void* stream);
// ---- weightp.hip
void mivc_launch_wp_stats(const uint8_t* y, const uint8_t* u, const uint8_t* v, int w, int h, int npics,
                          unsigned long long* out, void* stream);
void mivc_launch_wp_stats16(const uint16_t* y, const uint16_t* u, const uint16_t* v, int w, int h, int npics,
                            unsigned long long* out, void* stream);
void mivc_launch_wp_src(const uint8_t* src, uint8_t* dst, const int* wt, int B, long long plane_bytes, void* stream);
int mivc_launch_wp_ref8(const uint8_t* ref, uint8_t* dst, const int* wt, int B, long long plane_bytes, void* stream);
// ---- mbtree.hip
void mivc_launch_mbtree(int B, int F, int lbw, int lbh, const int* blk_cost, const int* blk_mv, void* prop,
                        float strength, float* out, void* stream);
// ---- lookahead.hip
long long mivc_lookahead_low_bytes(int w, int h, int N);
long long mivc_lookahead_quarter_bytes(int w, int h, int N);
int mivc_launch_lookahead(const uint8_t* y, int w, int h, long long fstride, int N, int F, uint8_t* low,
                          unsigned long long* frame_cost, int* blk_cost, int* blk_mv, int range, void* stream,
                          uint8_t* low4, int* mv4, unsigned long long* cost4, float* wt, unsigned long long* wstats,
                          float thr_mean, float thr_scale, int stage);
int mivc_launch_lookahead_multi(const uint8_t* low, int w, int h, int N, int F, const int* blk_cost, const int* blk_mv,
                                int D, int range, unsigned long long* out, void* stream, const float* wt);
// ---- metrics.hip
void mivc_launch_trellis_blocks(const int* w, int* out, int n, int qp, int mode, int skip_dc, void* stream);
void mivc_launch_satd_blocks(const uint8_t* src, const uint8_t* pred, int* out, int n, int mode, void* stream);
void mivc_launch_sse(int B, int W, int H, int w, int h, const uint8_t* sy, const uint8_t* su, const uint8_t* sv,
                     const uint8_t* ry, const uint8_t* ru, const uint8_t* rv, unsigned long long* sse,
                     float* ssim_sum, void* stream, const void* route, int nbuf);
// ---- hevc_intra.hip
void mivc_launch_hevc_intra(int B, int W, int H, const uint16_t* sy, const uint16_t* su, const uint16_t* sv,
                            uint16_t* ry, uint16_t* ru, uint16_t* rv, void* ctu, void* cu, int16_t* cy, int16_t* cu_,
                            int16_t* cv, const int* qp, const int8_t* run, int* cand, int bd, int analyze, int recon,
                            int* err, int sdh, const uint8_t* ctb_mask, void* stream, int ctu64, int rdoq, int rdoq_lam,
                            int slices, unsigned long long* tsmap, const int* ts_lamq, int* ts_count);
// ---- hevc_inter.hip
void mivc_launch_hevc_inter(int B, int W, int H, const uint16_t* sy, const uint16_t* su, const uint16_t* sv,
                            const uint16_t* fy, const uint16_t* fu, const uint16_t* fv, uint16_t* ry, uint16_t* ru,
                            uint16_t* rv, void* ctu, void* cu, int16_t* cy, int16_t* cu_, int16_t* cv, const int* qp,
                            const int8_t* run, const int* cand, const int16_t* mv, const int* me_cost, int bd,
                            int tu_split, int sdh, int intra_bias, void* stream, const int16_t* mvb,
                            const uint8_t* dirb, const uint16_t* f1y, const uint16_t* f1u, const uint16_t* f1v,
                            const int16_t* wp, const uint16_t* const* xref, const int16_t* mv8, int rdoq, int rdoq_lam,
                            const int16_t* wpb, const int* rd_lamq, unsigned long long* tsmap, const int* ts_lamq,
                            int* ts_count);
// ---- hevc_merge.hip
void mivc_launch_hevc_merge_refine(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref, const uint8_t* hp,
                                   const int16_t* mv_in, int16_t* mv_out, int* cost, const int16_t* pm, const int* qp,
                                   const int8_t* aq, void* stream, int ctu64, int slices);
void mivc_launch_hevc_b(int mode, int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref0, const uint8_t* ref1,
                        const uint8_t* hp0, const uint8_t* hp1, const int16_t* mv0, const int16_t* mv1, const int* cost0,
                        const int* cost1, const int16_t* pm0, const int16_t* pm1, const int16_t* tmv, const uint8_t* tdir,
                        const int16_t* mvb_in, const uint8_t* dir_in, int16_t* mvb_out, uint8_t* dir_out, int* cost,
                        int* bits, const int* qp, const int8_t* aq, void* stream, int bslice, int max_merge, int ctu64,
                        const uint8_t* chg_in, uint8_t* chg_out, int nref0, const uint8_t* const* xref,
                        const uint8_t* const* xhp, const int16_t* xmv, const int* xcost, const int16_t* xpm, int slices);
// ---- hevc_filters.hip
int mivc_launch_hevc_prep_frame(int B, const void* sy, const void* su, const void* sv, long long ss_y, long long ss_c,
                                int pitch_y, int pitch_c, int bps, int w, int h, uint16_t* dy, uint16_t* du,
                                uint16_t* dv, uint8_t* d8, int W, int H, int shift, int bd, void* stream);
int mivc_launch_hevc_proxy8(const uint16_t* src, uint8_t* dst, long long n, int shift, void* stream);
void mivc_launch_hevc_deblock(int B, int W, int H, int bd, uint16_t* y, uint16_t* u, uint16_t* v, const void* cu,
                              const void* ctu, const int8_t* run, void* stream);
void mivc_launch_hevc_sao(int B, int W, int H, int bd, const uint16_t* dy, const uint16_t* du, const uint16_t* dv,
                          uint16_t* y, uint16_t* u, uint16_t* v, const uint16_t* sy, const uint16_t* su,
                          const uint16_t* sv, void* ctu, const int* qp, const int8_t* run, int enable, void* stream,
                          int ctu64);
void mivc_launch_hevc_aq(int B, int W, int H, int bd, const uint16_t* sy, const uint16_t* su, const uint16_t* sv,
                         const int* qp, float strength, const float* extra, long long extra_stride, int extra_rows,
                         int* ctb_qp, int8_t* mb_aq, void* stream);
void mivc_launch_hevc_aq_terms(int B, int W, int H, int bd, const uint16_t* sy, const uint16_t* su, const uint16_t* sv,
                               float* terms, void* stream);
void mivc_launch_hevc_aq_auto_finish(int B, int W, int H, const float* terms, const int* qp, int mode, float strength,
                                     const float* extra, long long extra_stride, int extra_rows, int* ctb_qp,
                                     int8_t* mb_aq, void* stream);
void mivc_launch_hevc_qp_fixup(int B, int W, int H, void* ctu, const void* cu, const int* qp, const int8_t* run,
                               int wpp, void* stream, int ctu64, int slices);
void mivc_launch_hevc_pack_levels(int B, int W, int H, const int16_t* cy, const int16_t* cb, const int16_t* cr,
                                  unsigned long long* nzmap, int* cnt, unsigned* off, long long cap_blocks, int16_t* out,
                                  int* err, void* stream);
// ---- hevc_entropy.hip
long long mivc_hevc_entropy_state_bytes(int W, int H);
long long mivc_hevc_entropy_ctx_bytes();
int mivc_launch_hevc_entropy(const void* pic, int B, const int* qp, const void* ctu, const void* cu, const void* col,
                             const unsigned long long* nzmap, const int16_t* cy, const int16_t* cb, const int16_t* cr,
                             uint8_t* state, long long state_bytes, uint8_t* out, unsigned cap, unsigned* sizes,
                             int* errs, unsigned long long* offs, unsigned long long* offs_host, uint8_t* dst,
                             unsigned long long dst_cap, int* overflow, void* stream, unsigned long long* prof,
                             int* gprog, void* gctx, const unsigned long long* tsmap);
// ---- hevc_decode.hip
int mivc_launch_hevc_decode(const mivc::gpu::HevcDecParams* p, int stage, void* stream);
// ---- hevc_mc_probe.hip, hevc_tq_probe.hip, hevc_rd_cbf_probe.hip, hevc_tskip_probe.hip (test probes)
int mivc_launch_hevc_mc_probe(int ncase, const uint16_t* ref0, const uint16_t* ref1, int pw, int ph, const int16_t* cases,
                              uint16_t* out, int nt, int n, int dir, int bd, int ww, int wo, int ww1, int wo1, int wb,
                              int lean, void* stream);
int mivc_launch_hevc_tq_probe(int nblk, const int* res, int16_t* lev, int* rec, int* flag, int log2n, int bd, int qp,
                              int intra, int dst, int scan, int sdh, int rdoq, int rdoq_lam, int mfma, void* stream);
int mivc_launch_hevc_rd_cbf_probe(int nblk, const uint16_t* src, const uint16_t* pred, int16_t* lev, uint16_t* rec, int* flag,
                                  long long* terms, int log2n, int bd, int qp, int sdh, int rdoq, int rdoq_lam, int lamq,
                                  void* stream);
int mivc_launch_hevc_tskip_probe(int nblk, const uint16_t* src, const uint16_t* pred, int16_t* lev, uint16_t* rec, int* flag,
                                 long long* terms, int bd, int qp, int intra, int dst, int scan, int sdh, int rdoq,
                                 int rdoq_lam, int lamq, void* stream);
}
