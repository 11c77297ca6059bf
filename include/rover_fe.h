/*
 * rover_fe.h -- C ABI of librover_fe.so: MI355X-native SuperPoint extractor + LightGlue matcher.
 *
 * This is the drop-in boundary for Rover-SLAM's learned front end.  Each entry point names the
 * reference interface it replaces (paths relative to the reference checkout):
 *
 *   rfe_init / rfe_destroy        SuperPointOnnxRunner::InitOrtEnv   src/Extractors/superpoint_onnx.cc:4-66
 *                                 LightGlueDecoupleOnnxRunner::InitOrtEnv  src/Matchers/lightglue_onnx.cpp:4-98
 *   rfe_load_weights              the two model paths: src/Extractors/SPextractor.cc:93 (superpoint.onnx),
 *                                 src/Matchers/lightglue_onnx.cpp:38 (lightglue_sim.onnx)
 *   rfe_extract_u8                NormalizeImage (src/Matchers/transform.cpp:3-17) +
 *                                 SuperPointOnnxRunner::Extractor_Inference (superpoint_onnx.cc:88-162,
 *                                 Session::Run at :133-136) + the tensor unpacking half of
 *                                 Extractor_PostProcess (superpoint_onnx.cc:165-255)
 *   rfe_match                     LightGlueDecoupleOnnxRunner::Matcher_Inference
 *                                 (lightglue_onnx.cpp:162-240, Session::Run at :210-214); inputs are the
 *                                 already normalised keypoints of Matcher_PreProcess (:140-159)
 *   rfe_match_fused               rfe_match + Matcher_PostProcess_fused (lightglue_onnx.cpp:396-482):
 *                                 fills vnMatches12 exactly like SPmatcher::MatchingPoints_onnx
 *                                 (src/Matchers/SPmatcher.cc:359-542)
 *   rfe_extract_match_stream      batched-frames mode (BASELINE config 4): extract B frames and match
 *                                 frame i with frame i+1, everything device resident
 *
 * Conventions: plain pointers and sizes only.  Functions return RFE_OK (0) or a negative
 * rfe_status; nothing throws across the boundary; rfe_last_error() gives the message
 * (the reference prints to std::cerr and returns EXIT_FAILURE, superpoint_onnx.cc:59-65).
 * A ctx is single-caller (not re-entrant); several ctxs may be used concurrently from different
 * threads (the reference gives each SPextractor / SPmatcher its own ORT session,
 * src/Tracking.cc:645-651, :70).  "_dev" variants take DEVICE pointers and are asynchronous on
 * the ctx stream; the plain variants take HOST pointers and return after the results are copied.
 *
 * There is no CPU fallback: every entry point fails with RFE_ERR_NO_DEVICE if no gfx950 GPU
 * can be opened.
 */
#ifndef ROVER_FE_H
#define ROVER_FE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rfe_ctx rfe_ctx;

typedef enum {
    RFE_OK = 0,
    RFE_ERR_INVALID = -1,    /* bad argument */
    RFE_ERR_NO_DEVICE = -2,  /* no HIP device / wrong arch */
    RFE_ERR_HIP = -3,        /* a HIP runtime call failed */
    RFE_ERR_IO = -4,         /* weight file problem */
    RFE_ERR_NO_WEIGHTS = -5, /* model used before weights were set */
    RFE_ERR_OOM = -6
} rfe_status;

#define RFE_DESC_DIM 256
#define RFE_KIND_SUPERPOINT 1
#define RFE_KIND_LIGHTGLUE 2

/* ---- lifetime ---- */
int rfe_init(int device, rfe_ctx** out);
void rfe_destroy(rfe_ctx* ctx);
const char* rfe_last_error(rfe_ctx* ctx); /* ctx may be NULL: last error of a failed rfe_init */
const char* rfe_version(void);

/* ---- weights: ONNX graph files, RFEW container files, or host blobs in the canonical layout ----
 * rfe_load_weights takes, per path, EITHER the reference's own model file -- onnxmodel/superpoint.onnx (src/Extractors/SPextractor.cc:92-94) /
 * onnxmodel/lightglue_sim.onnx (src/Matchers/lightglue_onnx.cpp:38): the initializers are re-packed into the canonical layout and the graph's
 * baked-in hyper-parameters (see rfe_hparams below) are read from its nodes, in C++ (rover-slam_amd/csrc/onnx_load.hip; no Python step, no
 * protobuf / onnx library); a graph whose constants cannot be read, or whose tensors cannot be placed, is refused with the reason
 * (RFE_ERR_IO, rfe_last_error) -- OR an RFEW container written by rover-slam_amd/onnx_weights.py / weights.py; the file's first four bytes
 * decide.  rfe_load_onnx insists on ONNX. */
int rfe_load_weights(rfe_ctx* ctx, const char* sp_path, const char* lg_path); /* either may be NULL */
int rfe_load_onnx(rfe_ctx* ctx, const char* sp_path, const char* lg_path);    /* either may be NULL */
int rfe_set_weights(rfe_ctx* ctx, int kind, const float* blob, int64_t count);
int64_t rfe_weight_count(int kind);
/* Read-only weights are shared inside a process: every ctx that loads the same blob on the same device uses one device
 * copy (the reference keeps 2-3 extractors and 3 matchers per process, each with a private session: src/Tracking.cc:645-651,
 * :70, src/LocalMapping.cc:45, src/LoopClosing.cc:46).  rfe_weights_id: opaque id of the copy a ctx uses (0 = none);
 * equal ids = shared copy. */
uint64_t rfe_weights_id(rfe_ctx* ctx, int kind);

/* ---- graph hyper-parameters (RFEW version 2; per ctx) ----
 * The reference's two model files carry constants that never appear in its C++: the extractor takes K from the SHAPE of the
 * `keypoints` output (src/Extractors/superpoint_onnx.cc:169-181) because max_num_keypoints, the detection threshold, the NMS
 * radius and the border width are baked into onnxmodel/superpoint.onnx at export time (src/Extractors/SPextractor.cc:92-94),
 * and the matcher reads whatever matches0 / mscores0 hold (src/Matchers/lightglue_onnx.cpp:404-409) because depth, heads and the
 * in-graph filter threshold are baked into onnxmodel/lightglue_sim.onnx (lightglue_onnx.cpp:38).  rover-slam_amd/onnx_weights.py
 * reads them from the graphs and writes them into the RFEW v2 header; rfe_load_weights applies them to the ctx.  Hyper-parameters belong
 * to a weight set: version-1 files and rfe_set_weights (bare blobs) carry none and RESET the loaded kind's values to the defaults below
 * (so a v2 load followed by rfe_set_weights does not keep the earlier file's radius / border / top-k rule); call rfe_set_hparams AFTER
 * the weights to state other values.
 *   sp_max_keypoints / sp_detection_threshold / lg_filter_threshold are what a drop-in caller passes as Kmax / thr / filter_thr
 *     (the C++ shims do exactly that); the entry points themselves keep taking them as arguments.
 *   sp_nms_radius (1..8) and sp_remove_borders (0..64) act inside rfe_extract_* (simple_nms window 2r+1, border set to -1).
 *   sp_topk_always: 0 = the published top_k_keypoints (score-descending order only when more than Kmax candidates pass, row-major
 *     otherwise); 1 = exports that run torch.topk(scores, min(k, n)) unconditionally (TopK behind a Min in the graph): keypoints
 *     always ordered by (score descending, pixel index ascending).
 *   lg_layers / lg_heads describe the file; the kernels are built for 9 layers of 4 heads x 64 and rfe_set_hparams /
 *     rfe_load_weights refuse anything else (RFE_ERR_INVALID / RFE_ERR_IO). */
typedef struct rfe_hparams {
    int32_t sp_max_keypoints;       /* default 1024 */
    float sp_detection_threshold;   /* default 0.0005 */
    int32_t sp_nms_radius;          /* default 4 */
    int32_t sp_remove_borders;      /* default 4 */
    int32_t sp_topk_always;         /* default 0 */
    int32_t lg_layers;              /* 9 */
    int32_t lg_heads;               /* 4 */
    float lg_filter_threshold;      /* default 0.1 */
} rfe_hparams;
int rfe_get_hparams(rfe_ctx* ctx, rfe_hparams* out);
int rfe_set_hparams(rfe_ctx* ctx, const rfe_hparams* in);

/* ---- options (per ctx; the library never reads the environment) ----
 * RFE_OPT_LG_FOLD_WO (default 1): every LightGlue attention output projection (Wo, bo) is multiplied into the message
 *   half of the following ffn.0 Linear at load time (W1 [x | ctx Wo^T + bo] + b1 = [W1a | W1b Wo] [x | ctx] + (b1 + W1b bo),
 *   formed in double precision): 18 fewer GEMM launches per forward (+4 % throughput).  Mathematically identical; the
 *   message is simply never rounded to fp32.  0 keeps the graph of lightglue_sim.onnx node for node.  Measured over 40
 *   cases at K = 1024 (profiles/r02_lg_tolerance.md): match lists identical either way; match scores move by <= 3.2e-4
 *   (folded) / <= 2.0e-4 (unfolded) against the fp32 CPU oracle, which itself sits up to 2.6e-4 from a float64 evaluation
 *   of the same graph (HIP vs float64: 2.4e-4 / 1.8e-4) -- the stated tolerance is 5e-4 for both.
 * RFE_OPT_LG_FP16X2 (default 0 = every LightGlue matrix product on the fp32 matrix instructions): 1 = the Linears (every call: the throughput
 *   tiles of batched calls, gemm_h2.hip, and the one- / few-pair latency tiles, gemm_lat.hip) AND the fused attention (batched calls of
 *   >= 32 768 token rows: lg_attention_h2.hip; one / few pairs: the split form of lg_attention_lat.hip) run as SPLIT products on the f16 matrix pipe --
 *   every fp32 operand as fp16 hi + fp16 lo (22 of 24 significand bits), three of the four cross products, fp32 accumulation, softmax
 *   and LayerNorm / GELU in fp32 as before (rover-slam_amd/csrc/gemm_h2.hip, lg_attention_h2.hip).  Stand-alone the Linears are
 *   2.2-2.8x and the attention 2.4-2.6x faster than the fp32 kernels; error against float64: Linears rms 3.2e-8 of sum|a||b| (fp32 fmaf
 *   chain: 2.8e-8), attention context 3.7e-6 (fp32 kernels: 4.8e-6) (profiles/r03_ab_notes.md, tests/test_gpu_attention.py); end to end
 *   over the 40-case study the match lists are identical and the scores sit 1.6e-4 (Wo folded) / 2.6e-4 (unfolded) from float64, inside
 *   the spread of the fp32 evaluations of the same graph (1.8e-4 .. 2.6e-4, profiles/r03_lg_tolerance.md).  Valid while activations
 *   stay below fp16's 65504 in magnitude (LightGlue's are O(1..100)); past it the attention's operands saturate (finite results), the
 *   Linears' inputs too (MODE.FP16_OVFL).  One pair per call: 2.43 -> 2.06 ms incl. both extractions, a stereo frame 2.59 -> 2.25 ms
 *   (bench.py `latency.resident_fp16x2`).  The assignment and all of SuperPoint stay fp32; bench.py reports the throughput step as
 *   `variants.fp16x2`, never as the headline. */
#define RFE_OPT_LG_FOLD_WO 1
#define RFE_OPT_LG_FP16X2 2
/* RFE_OPT_HOST_GRAPH (default 0): the synchronous host entries (rfe_extract_u8 / _bin / _f32, rfe_match / rfe_match_fused) submit their kernel sequence as ONE
 *   replayed hipGraph per call shape instead of 17 .. 100 stream launches (captured on the THIRD call of a shape, four shapes kept per entry, least recently
 *   used replaced; weights, hyper-parameters, options, workspaces and shape are part of the key; profiling falls back).  For rfe_match the shape holds Mmax
 *   and Nmax, so the option only helps FIXED-CAPACITY callers (keypoint counts that saturate, or are padded to, a capacity): a caller whose counts differ on
 *   every frame never repeats a shape, is never captured and gets ordinary launches.  Results are identical.  The device is busy for 98 % of a one-pair call either way, so the median
 *   does not move; the option is there for hosts whose threads get preempted inside the enqueue burst (tail latency).  Measured: profiles/r05_ab_notes.md. */
#define RFE_OPT_HOST_GRAPH 3
int rfe_set_option(rfe_ctx* ctx, int option, int value);
int rfe_get_option(rfe_ctx* ctx, int option, int* value);

/* ---- stream / sync / device memory helpers (so a pure-C caller needs no HIP headers) ---- */
int rfe_set_stream(rfe_ctx* ctx, void* hip_stream); /* NULL -> ctx's own stream */
int rfe_synchronize(rfe_ctx* ctx);
int rfe_malloc(rfe_ctx* ctx, size_t bytes, void** dev_ptr);
int rfe_free(rfe_ctx* ctx, void* dev_ptr);
/* Pinned (page-locked, portable) host memory.  Optional: every host entry point takes ANY host pointer.  When the descriptor output of
 * rfe_extract_u8 / rfe_extract_f32 / rfe_extract_u8_bin lies inside a block from rfe_host_malloc, the K x 256 floats are DMA'd straight into it
 * (otherwise they are staged through the ctx's pinned block and copied on the host: ~1 MB per 1024-keypoint frame).  The C++ runner shim
 * keeps its output tensors in such blocks.  Not tied to a ctx; rfe_host_free(NULL) is a no-op. */
int rfe_host_malloc(size_t bytes, void** host_ptr);
void rfe_host_free(void* host_ptr);
/* bytes of device workspace the ctx holds right now (grow-only: the high-water mark of every call so far; weights not included) */
int64_t rfe_workspace_bytes(rfe_ctx* ctx);
int rfe_memcpy_h2d(rfe_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int rfe_memcpy_d2h(rfe_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- SuperPoint ----
 * img:   u8 grayscale, B frames of H x W, row pitch `stride` bytes, frame pitch stride*H
 *        (any H, W >= 8, as the reference graph's dynamic axes allow: the three 2x2 max-pools floor, keypoints come from
 *        the 8*(H/8) x 8*(W/8) top-left frame -- KITTI's 1241 x 376 gives a 1240 x 376 score map; the reference asserts
 *        CV_8UC1, SPextractor.cc:525)
 * Kmax:  capacity per frame (the export-time max_num_keypoints of the reference graph)
 * thr:   detection threshold (0.0005 in the LightGlue-ONNX SuperPoint export)
 * n:     [B]            number of keypoints per frame
 * kxy:   [B,Kmax,2] i32 (x,y) integer pixel coordinates; rows >= n[b] are zero
 * score: [B,Kmax]
 * desc:  [B,Kmax,256]   L2-normalised descriptors
 * Order: score-descending (ties: row-major pixel index ascending) when more than Kmax candidates
 * pass the threshold, row-major otherwise. */
int rfe_extract_u8(rfe_ctx* ctx, const uint8_t* img, int H, int W, int stride, int B, int Kmax,
                   float thr, int32_t* n, int32_t* kxy, float* score, float* desc);
int rfe_extract_u8_dev(rfe_ctx* ctx, const uint8_t* img_dev, int H, int W, int stride, int B,
                       int Kmax, float thr, int32_t* n_dev, int32_t* kxy_dev, float* score_dev,
                       float* desc_dev);

/* The float entry: img is an ALREADY normalised single-channel float image (what NormalizeImage produced, or any CV_32F the
 * caller hands to Extractor_Inference, src/Extractors/superpoint_onnx.cc:88-118); the values enter conv1a unchanged, whatever
 * their range.  stride in floats.  For img[i] = u8[i] * (1/255.f) the outputs are bit-identical to rfe_extract_u8's. */
int rfe_extract_f32(rfe_ctx* ctx, const float* img, int H, int W, int stride, int B, int Kmax,
                    float thr, int32_t* n, int32_t* kxy, float* score, float* desc);
int rfe_extract_f32_dev(rfe_ctx* ctx, const float* img_dev, int H, int W, int stride, int B,
                        int Kmax, float thr, int32_t* n_dev, int32_t* kxy_dev, float* score_dev,
                        float* desc_dev);

/* The same with a second descriptor output for the loop-closure side: desc_bin u8 [B,Kmax,256] = desc > 0,
 * i.e. Frame::binarize_descriptors (src/Frame.cc:1034-1043) written by the sampling kernel itself, ready for
 * Converter::toDescriptorVector + the DBoW3 vocabulary of Frame::ComputeBoW3 (:1044-1054), which stay on the CPU.
 * desc_bin may be NULL (= the plain call). */
int rfe_extract_u8_bin(rfe_ctx* ctx, const uint8_t* img, int H, int W, int stride, int B, int Kmax, float thr, int32_t* n,
                       int32_t* kxy, float* score, float* desc, uint8_t* desc_bin);
int rfe_extract_u8_bin_dev(rfe_ctx* ctx, const uint8_t* img_dev, int H, int W, int stride, int B, int Kmax, float thr,
                           int32_t* n_dev, int32_t* kxy_dev, float* score_dev, float* desc_dev, uint8_t* desc_bin_dev);

/* ---- SuperPoint on a scale pyramid (SPextractor with nlevels > 1) ----
 * The reference's ExtractMultiLayers (src/Extractors/SPextractor.cc:619-653) over the levels of ComputePyramid (:686-712): level l is
 * W_l x H_l = lrintf((float)W * (1.0f / s_l)) x lrintf((float)H * (1.0f / s_l)) (src/Extractors/SPextractor.cc:691-692), s_0 = 1,
 * s_l = (float)((double)s_{l-1} * scale_factor) (the constructor, src/Extractors/SPextractor.cc:109-129; its per-level feature budget
 * mnFeaturesPerLevel, :133-146, is what a caller passes as kmax), made from level l-1 by 11-bit
 * fixed-point bilinear resampling with half-pixel centres (modelled on cv::resize INTER_LINEAR; bit parity with OpenCV is NOT claimed).
 * Every level runs the rfe_extract_u8 pipeline with Kmax = kmax[l] (a level below 8 px or with kmax[l] == 0 yields no keypoints), and
 * the rows are merged per frame in level order: row i of level l lands at sum_{j<l} n_j + i with kpts = (x * s_l, y * s_l) (one fp32
 * multiply, keypoint.pt *= mvScaleFactor[level]), octave = l, score / desc unchanged.
 * rfe_pyramid_geometry: pure function, no device (like rfe_pool_shard): the level sizes and scale factors; RFE_ERR_INVALID for arguments
 * rfe_extract_pyramid_u8 refuses (the arrays are still filled when only a level rounds to zero pixels). */
#define RFE_MAX_LEVELS 16
int rfe_pyramid_geometry(int H, int W, int nlevels, float scale_factor, int32_t* level_h, int32_t* level_w, float* level_scale);
/* B frames of H x W (row pitch stride, frame pitch stride*H); kmax [nlevels] is a HOST array; Ktot = sum of kmax.
 * n [B], level_n [B,nlevels] (may be NULL), kpts [B,Ktot,2] f32 level-0 pixels, octave [B,Ktot] i32, score [B,Ktot],
 * desc [B,Ktot,256]; levels [B, sum_l H_l*W_l] u8, level 0 first, tight pitch (may be NULL).  Rows >= n[b] are zero.
 * Refused (RFE_ERR_INVALID): nlevels outside 1..16; scale_factor <= 1 or > 4 when nlevels > 1; a kmax[l] outside 0..4096, or all 0;
 * H or W below 8, B below 1, stride below W; a NULL required pointer; a level that rounds to zero pixels.
 * RFE_OPT_HOST_GRAPH does not apply to these entries (their kernel sequence is submitted the ordinary way).  The first call of an
 * (H, W, nlevels, scale_factor) uploads its resampling tables and synchronises the ctx stream, as a workspace growth does. */
int rfe_extract_pyramid_u8(rfe_ctx* ctx, const uint8_t* img, int H, int W, int stride, int B, int nlevels, float scale_factor,
                           const int32_t* kmax, float thr, int32_t* n, int32_t* level_n, float* kpts, int32_t* octave,
                           float* score, float* desc, uint8_t* levels);
/* The same with device pointers (except kmax), asynchronous on the ctx stream: no host synchronisation and no host read of device
 * data after the first call of a shape.  With `levels`, the pyramid is built there and SuperPoint reads levels >= 1 from it. */
int rfe_extract_pyramid_u8_dev(rfe_ctx* ctx, const uint8_t* img_dev, int H, int W, int stride, int B, int nlevels, float scale_factor,
                               const int32_t* kmax, float thr, int32_t* n_dev, int32_t* level_n_dev, float* kpts_dev,
                               int32_t* octave_dev, float* score_dev, float* desc_dev, uint8_t* levels_dev);

/* ---- LightGlue ----
 * P pairs.  k0n/k1n: normalised keypoints [P,Mmax,2] / [P,Nmax,2]; d0/d1: [P,Mmax,256] /
 * [P,Nmax,256]; m/n: [P] valid counts.  filter_thr: in-graph match filter (0.1).
 * S: [P] number of matches; pairs: [P,min(Mmax,Nmax),2] (i,j) with i ascending; ms: scores. */
int rfe_match(rfe_ctx* ctx, const float* k0n, const float* k1n, const float* d0, const float* d1,
              const int32_t* m, const int32_t* n, int P, int Mmax, int Nmax, float filter_thr,
              int32_t* S, int32_t* pairs, float* ms);
int rfe_match_dev(rfe_ctx* ctx, const float* k0n, const float* k1n, const float* d0,
                  const float* d1, const int32_t* m, const int32_t* n, int P, int Mmax, int Nmax,
                  float filter_thr, int32_t* S, int32_t* pairs, float* ms);

/* One pair, pixel keypoints in, vnMatches12 out (length M, -1 = unmatched); returns the number
 * of accepted matches (>= 0) or a negative rfe_status.  (rows, cols) is the image size used by
 * NormalizeKeypoints (src/Matchers/transform.cpp:19-32); pass 300,400 to reproduce the hard-coded quirk of three of the reference's
 * four overloads (SPmatcher.cc:360-361,376-377,414-415). */
int rfe_match_fused(rfe_ctx* ctx, const float* kpts0_xy, int M, const float* kpts1_xy, int N,
                    const float* desc0, const float* desc1, int rows, int cols, float filter_thr,
                    float match_thresh, int32_t* vnMatches12);

/* ---- batched stream (device resident): extract B frames, match (i, i+1) for i < B-1 ----
 * Outputs as in rfe_extract_u8_dev, plus S:[B-1], pairs:[B-1,Kmax,2], ms:[B-1,Kmax]
 * (any match output pointer may be NULL to skip the copy-out of that array). */
int rfe_extract_match_stream_dev(rfe_ctx* ctx, const uint8_t* img_dev, int H, int W, int stride,
                                 int B, int Kmax, float thr, float filter_thr, int32_t* n_dev,
                                 int32_t* kxy_dev, float* score_dev, float* desc_dev,
                                 int32_t* S_dev, int32_t* pairs_dev, float* ms_dev);

/* ---- sparse stereo matching ----
 * Frame::ComputeStereoMatches (src/Frame.cc:1159-1446) for nLevels == 1 (rfe_stereo_match_pyramid below for nLevels > 1): for every left keypoint, best right
 * keypoint within +-2 rows and the disparity range [0, mbf/mb) by 256-d L2 distance
 * (SPmatcher::DescriptorDistance_sp, src/Matchers/SPmatcher.cc:2184-2189; accepted below (TH_HIGH+TH_LOW)/2 = 1.3, SPmatcher.cc:13-14),
 * 11x11 SAD refinement over +-5 px on the raw images, parabola sub-pixel fit, median outlier cut.
 * kL/kR: pixel keypoints [N,2]/[Nr,2]; dL/dR: descriptors [N,256]/[Nr,256]; mb, mbf: baseline (m) and
 * baseline*fx of the Frame.  Outputs mvuRight / mvDepth: [N], -1 = no match.  Deviation: left keypoints whose
 * 11x11 patch leaves the image are skipped (the reference's cv::Mat::rowRange would throw). */
int rfe_stereo_match(rfe_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride,
                     const float* kL, int N, const float* kR, int Nr, const float* dL, const float* dR,
                     float mb, float mbf, float* uRight, float* depth);
int rfe_stereo_match_dev(rfe_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride,
                         const float* kL, int N, const float* kR, int Nr, const float* dL, const float* dR,
                         float mb, float mbf, float* uRight, float* depth);

/* ---- stereo stream (BASELINE configs[4]): ONE device-resident call per stereo frame ----
 * What the reference does per stereo frame, fused: the stereo Frame constructor extracts the left and right views on two
 * threads (src/Frame.cc:106-171, :142-147) and calls ComputeStereoMatches (:165, :1159-1446); Tracking then matches the
 * frame against the previous one with LightGlue (SPmatcher::MatchingPoints_onnx, Frame overload, src/Matchers/SPmatcher.cc:457-542,
 * called from :1050-1080).  Here: both views through SuperPoint as one batch of 2, the sparse stereo match on the device-
 * resident features (keypoint counts never visit the host), and one LightGlue match of THIS left view (set 0) against the
 * PREVIOUS left view (set 1, kept inside the ctx) with the true image size -- the argument order of
 * SearchBySP(mCurrentFrame, mLastFrame) (src/Tracking.cc:3465; SPmatcher.cc:1050-1054), so pairs[k] = (index in the current
 * frame, index in the previous frame) like vnMatches1[IdxCF] = IdxLF.  Asynchronous on the ctx stream.
 * imgL/imgR: device u8 [H,W], row pitch `stride`.  reset != 0 (or a change of H, W, Kmax) starts a new sequence: S = 0.
 * Outputs (device): n [2] (left, right), kxy [2,Kmax,2], score [2,Kmax], desc [2,Kmax,256] as rfe_extract_u8_dev;
 * uRight / depth [Kmax] as rfe_stereo_match (entries >= n[0] are -1); S [1], pairs [Kmax,2], ms [Kmax] as rfe_match_dev. */
int rfe_stereo_frame_dev(rfe_ctx* ctx, const uint8_t* imgL_dev, const uint8_t* imgR_dev, int H, int W, int stride, int Kmax,
                         float thr, float filter_thr, float mb, float mbf, int reset, int32_t* n_dev, int32_t* kxy_dev,
                         float* score_dev, float* desc_dev, float* uRight_dev, float* depth_dev, int32_t* S_dev,
                         int32_t* pairs_dev, float* ms_dev);

/* ---- octave-aware sparse stereo matching: scale-pyramid keypoints (SPextractor with nlevels > 1) ----
 * Frame::ComputeStereoMatches (src/Frame.cc:1159-1446) with its four uses of the scale pyramid: the row band of a RIGHT keypoint is
 * r = 2 * mvScaleFactors[kpR.octave] (:1207-1218), a candidate's octave lies within +-1 of the left keypoint's (:1273), the SAD
 * refinement runs at the left keypoint's level on coordinates round(pt * mvInvScaleFactors[octave]) (:1302-1307), and the result
 * goes back to level 0 with mvScaleFactors[octave] (:1405).  Everything else is rfe_stereo_match, and with nlevels == 1 the outputs
 * are rfe_stereo_match's bit for bit.
 * levelsL / levelsR: ONE view's level images each, exactly the `levels` output of rfe_extract_pyramid_u8[_dev] ([sum_l H_l*W_l] u8,
 * level 0 first, tight pitch; with B = 2 the second view starts sum_l H_l*W_l bytes after the first).  The library recomputes the
 * geometry from (H, W, nlevels, scale_factor) as rfe_pyramid_geometry does; the caller passes no tables.
 * kL/kR: [N,2]/[Nr,2] f32 level-0 pixels, octL/octR: [N]/[Nr] i32, dL/dR: [N,256]/[Nr,256]; uRight / depth: [N], -1 = no match.
 * sad_source: which image the 11x11 patches come from.  ORB-SLAM3 reads mvImagePyramid[kpL.octave]; Rover-SLAM commented that out
 * (src/Frame.cc:1315, :1341) and reads level 0 at the level-scaled coordinates, a different place for octave > 0 (DESIGN.md 6c has
 * the comparison).  Both are offered; the bounds checks use the size of the image that is read.
 * Refused (RFE_ERR_INVALID): geometry arguments rfe_pyramid_geometry refuses; a sad_source other than the two; N or Nr outside 0..4096
 * (the outlier cut sorts in one workgroup); mb <= 0; a NULL required pointer; host entry only: an octave outside [0, nlevels).  The
 * _dev entry cannot read the octaves without a synchronisation: there, a left keypoint with such an octave gets no match and a right
 * one is never a candidate. */
#define RFE_STEREO_SAD_LEVEL  0   /* patches from pyramid level kpL.octave (ORB-SLAM3; default) */
#define RFE_STEREO_SAD_LEVEL0 1   /* patches from level 0 at level-scaled coordinates (Rover-SLAM src/Frame.cc:1318,1356 as written) */
int rfe_stereo_match_pyramid(rfe_ctx* ctx, const uint8_t* levelsL, const uint8_t* levelsR, int H, int W, int nlevels, float scale_factor,
                             const float* kL, const int32_t* octL, int N, const float* kR, const int32_t* octR, int Nr,
                             const float* dL, const float* dR, float mb, float mbf, int sad_source, float* uRight, float* depth);
/* the same with device pointers, asynchronous on the ctx stream */
int rfe_stereo_match_pyramid_dev(rfe_ctx* ctx, const uint8_t* levelsL, const uint8_t* levelsR, int H, int W, int nlevels, float scale_factor,
                                 const float* kL, const int32_t* octL, int N, const float* kR, const int32_t* octR, int Nr,
                                 const float* dL, const float* dR, float mb, float mbf, int sad_source, float* uRight, float* depth);
/* rfe_stereo_frame_dev for pyramids, ONE device-resident call per stereo frame: both views through the pyramid extraction as one
 * batch of 2 (rfe_extract_pyramid_u8_dev's outputs: n [2], level_n [2,nlevels] or NULL, kpts [2,Ktot,2], octave [2,Ktot],
 * score [2,Ktot], desc [2,Ktot,256]), the octave-aware stereo match on the device-resident merged features (uRight / depth [Ktot],
 * entries >= n[0] are -1), and one LightGlue match of THIS left view (set 0) against the PREVIOUS left view (set 1) on
 * NormalizeKeypoints of the float level-0 keypoints with the true image size (S [1], pairs [Ktot,2], ms [Ktot]).
 * kmax: HOST array [nlevels], Ktot = sum <= 4096.  reset != 0, a change of H, W, nlevels, scale_factor or any kmax[l], or an
 * rfe_stereo_frame_dev call on the same ctx in between, starts a new sequence (S = 0): the two entries never match against each
 * other's stored view.  No host synchronisation and no host read of device data after the first call of a shape;
 * RFE_OPT_HOST_GRAPH does not apply.  Refusals: those of rfe_extract_pyramid_u8_dev and rfe_stereo_match_pyramid, Ktot > 4096. */
int rfe_stereo_frame_pyramid_dev(rfe_ctx* ctx, const uint8_t* imgL_dev, const uint8_t* imgR_dev, int H, int W, int stride,
                                 int nlevels, float scale_factor, const int32_t* kmax, float thr, float filter_thr, float mb, float mbf,
                                 int sad_source, int reset, int32_t* n_dev, int32_t* level_n_dev, float* kpts_dev, int32_t* octave_dev,
                                 float* score_dev, float* desc_dev, float* uRight_dev, float* depth_dev, int32_t* S_dev,
                                 int32_t* pairs_dev, float* ms_dev);

/* ---- descriptor helpers for the callers' classic searches, host pointers (device forms below) ----
 * rfe_l2_distance_matrix: out[i*N + j] = SPmatcher::DescriptorDistance_sp(a_i, b_j)
 *   (src/Matchers/SPmatcher.cc:2184-2189) for all pairs of a [M,256] x b [N,256]; the candidate lists of
 *   SearchByProjection / Fuse (SPmatcher.cc:1170-1354, 49-357) stay with the caller.
 * rfe_binarize_descriptors: Frame::binarize_descriptors (src/Frame.cc:1034-1043): out u8 [rows,256] = desc > 0. */
int rfe_l2_distance_matrix(rfe_ctx* ctx, const float* a, int M, const float* b, int N, float* out);
int rfe_binarize_descriptors(rfe_ctx* ctx, const float* desc, int rows, uint8_t* out);

/* rfe_search_candidates: the best / second-best descriptor scan of SPmatcher::SearchByProjection1
 *   (src/Matchers/SPmatcher.cc:1218-1248; the same loop in SearchByProjection :755-800 and Fuse :150-200) for Nq
 *   map-point descriptors q [Nq,256] against the frame descriptors f [Nf,256].  Candidate lists are the caller's
 *   (Frame::GetFeaturesInArea) in CSR form: cand[offsets[i] .. offsets[i+1]) are the frame features near map point i,
 *   scanned in that order.  skip [Nf] (may be NULL): non-zero = feature already owns a MapPoint with observations
 *   (:1226-1228).  Per map point: best_idx (-1 = none), best_dist and second_dist (both start at 256, strict '<').
 *   The TH_HIGH cut and the greedy assignment (:1253-1262) stay with the caller.
 * rfe_distinctive_descriptors: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438-530) for Np map points at
 *   once: desc holds the observed descriptors of all points back to back, offsets [Np+1] delimits them (<= 8192 per
 *   point).  best[p] = index within the point's own list of the descriptor with the least median distance to the
 *   others (first strict minimum, -1 for an empty point), median[p] = that median. */
int rfe_search_candidates(rfe_ctx* ctx, const float* q, int Nq, const float* f, int Nf, const int32_t* offsets,
                          const int32_t* cand, const uint8_t* skip, int32_t* best_idx, float* best_dist, float* second_dist);
int rfe_distinctive_descriptors(rfe_ctx* ctx, const float* desc, const int32_t* offsets, int Np, int32_t* best, float* median);

/* Device-resident forms of the four helpers above (descriptors normally never leave HBM: they come out of rfe_extract_u8_dev /
 * rfe_stereo_frame_dev, and the host forms re-upload 1 KB per descriptor per call): every pointer is a DEVICE pointer, the call is
 * asynchronous on the ctx stream, the host forms are thin staging wrappers around these.  What the host forms validate and these
 * cannot without a synchronisation is the caller's contract instead: offsets[0] = 0, offsets non-decreasing;
 * rfe_search_candidates_dev ignores candidate indices outside [0, Nf) (SPmatcher.cc:1218-1262 semantics otherwise unchanged);
 * rfe_distinctive_descriptors_dev (MapPoint.cc:438-530) takes `total` >= offsets[Np] (descriptor count) and `maxn` >= the largest
 * observation count of any point (<= 8192) from the caller, and reports a point with more observations than maxn rounded up to
 * a power of two as best = -2. */
int rfe_l2_distance_matrix_dev(rfe_ctx* ctx, const float* a_dev, int M, const float* b_dev, int N, float* out_dev);
int rfe_binarize_descriptors_dev(rfe_ctx* ctx, const float* desc_dev, int rows, uint8_t* out_dev);
int rfe_search_candidates_dev(rfe_ctx* ctx, const float* q_dev, int Nq, const float* f_dev, int Nf, const int32_t* offsets_dev,
                              const int32_t* cand_dev, const uint8_t* skip_dev, int32_t* best_idx_dev, float* best_dist_dev,
                              float* second_dist_dev);
int rfe_distinctive_descriptors_dev(rfe_ctx* ctx, const float* desc_dev, const int32_t* offsets_dev, int Np, int total, int maxn,
                                    int32_t* best_dev, float* median_dev);

/* ---- SPmatcher::SearchByProjection1 as one call ----
 * The left-camera branch of SearchByProjection1 (src/Matchers/SPmatcher.cc:1190-1283), which Tracking::SearchLocalPoints runs on every
 * tracked frame, from the projected map points to what the loop leaves in F.mvpMapPoints: the feature grid (Frame::AssignFeaturesToGrid /
 * PosInGrid, src/Frame.cc:488-523, 998-1014; 32 x 24 cells over [min_x, max_x) x [min_y, max_y) = mnMinX..mnMaxY, cell = roundf), the
 * candidate list of every map point (Frame::GetFeaturesInArea, src/Frame.cc:895-987, in its visiting order: cell column, cell row,
 * feature index), the best / second-best scan of rfe_search_candidates over it, and the loop's SEQUENTIAL assignment: map points are
 * processed in index order, feature j is blocked for map point i when skip[j] != 0 (it owned an observed MapPoint before the call) or
 * when a map point k < i with observed[k] != 0 was accepted on j; map point i is accepted when its best distance <= th_high (the
 * reference's TH_HIGH is 1.4f).  The result is exact, not an approximation of the loop.
 *   q [Nq,256] map-point descriptors, proj [Nq,2] (mTrackProjX, mTrackProjY), radius [Nq] the final window half size
 *   (RadiusByViewingCos * th * mvScaleFactors[level]; a feature is a candidate when |dx| < radius and |dy| < radius, both strict),
 *   pred_level [Nq] or NULL = 0 (a feature passes with pred_level - 1 <= octave <= pred_level), observed [Nq] or NULL = all 1
 *   (Observations() > 0 of the map point);
 *   f [Nf,256] frame descriptors; the feature positions as EXACTLY ONE of kpts [Nf,2] f32 (mvKeysUn, the pyramid entries' output) and
 *   kxy [Nf,2] i32 (rfe_extract_u8_dev / rfe_stereo_frame_dev's output, read as float); octave [Nf] or NULL = 0; skip [Nf] or NULL.
 *   assign [Nf]: the LAST accepted map point whose best feature is this one (an unobserved earlier writer is overwritten), -1 = none;
 *   best_idx / best_dist / second_dist [Nq] (each may be NULL): what map point i saw at its turn, best_idx even when best_dist > th_high
 *   (-1 / 256 / 256 without an unblocked candidate); stats [4]: accepted map points (overwritten ones count, as the reference's
 *   nmatches), candidates over all lists, rounds the assignment took, overflow flag.
 * rfe_search_by_projection_dev: DEVICE pointers, asynchronous on the ctx stream; no host synchronisation and no host read of device data
 *   once the workspace has its size.  nf_dev (device [1], or NULL): the feature count is min(*nf_dev, Nf), read on the device -- the n
 *   rfe_stereo_frame_dev leaves there; rows past it are never candidates and their assign is -1.  cand_cap: (index, distance) slots for
 *   all lists together, kept in the ctx workspace.  When the lists need more the call still completes inside its buffers: stats[3] = 1,
 *   stats[1] = the slots needed, every assign / best_idx -1, every distance 256, stats[0] = 0.  stats is required.  A non-finite
 *   projection or radius, or a pred_level outside 0..RFE_MAX_LEVELS-1, gives that map point an empty list.
 * rfe_search_by_projection: HOST pointers; sizes the slots itself (never reports overflow; stats may be NULL) and returns stats[0] >= 0.
 * Refused (RFE_ERR_INVALID): Nq outside 0..16384; Nf outside 0..4096; max_x <= min_x or max_y <= min_y; cand_cap < 0; both or neither of
 *   kpts / kxy; a NULL required pointer; host form only: a pred_level outside 0..RFE_MAX_LEVELS-1, a non-finite projection, radius,
 *   keypoint, bound or th_high.  Nq == 0 or Nf == 0 is valid (nothing matches).
 * Out of scope: the right-camera branch of two-camera rigs (:1285-1351) -- the caller keeps it. */
int rfe_search_by_projection_dev(rfe_ctx* ctx, const float* q_dev, const float* proj_dev, const float* radius_dev,
                                 const int32_t* pred_level_dev, const uint8_t* observed_dev, int Nq, const float* f_dev,
                                 const float* kpts_dev, const int32_t* kxy_dev, const int32_t* octave_dev, const uint8_t* skip_dev, int Nf,
                                 const int32_t* nf_dev, float min_x, float min_y, float max_x, float max_y, float th_high, int cand_cap,
                                 int32_t* assign_dev, int32_t* best_idx_dev, float* best_dist_dev, float* second_dist_dev,
                                 int32_t* stats_dev);
int rfe_search_by_projection(rfe_ctx* ctx, const float* q, const float* proj, const float* radius, const int32_t* pred_level,
                             const uint8_t* observed, int Nq, const float* f, const float* kpts, const int32_t* kxy, const int32_t* octave,
                             const uint8_t* skip, int Nf, float min_x, float min_y, float max_x, float max_y, float th_high,
                             int32_t* assign, int32_t* best_idx, float* best_dist, float* second_dist, int32_t* stats);

/* ---- the Sim3 SearchByProjection overloads of loop closing as one call ----
 * SPmatcher::SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming)
 * (src/Matchers/SPmatcher.cc:1558-1669) and SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) (:2076-2182),
 * which LoopClosing runs several times per loop / merge candidate: the front of the loop (transform, projection, the four gates,
 * MapPoint::PredictScale, the radius) in one kernel, then the grid, candidate lists (KeyFrame::GetFeaturesInArea: no octave gate), scan and
 * sequential assignment of rfe_search_by_projection with every map point observed: a feature is blocked when matched_in[f] != 0 or an
 * earlier accepted map point took it.  All arithmetic is fp32 in the order the reference writes it, without contraction; the pose is the
 * caller's (the device derives none): Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) as :1566 builds it.
 *   rfe_sim3_params: quat = Tcw.unit_quaternion() as (x, y, z, w), t = Tcw.translation(), ow = Tcw.inverse().translation(); pinhole
 *   fx, fy, cx, cy; the keyframe's mnMinX, mnMinY, mnMaxX, mnMaxY; th (an int in the reference); nlevels = mnScaleLevels (1..RFE_MAX_LEVELS),
 *   log_scale_factor = mfLogScaleFactor, scale_factors = mvScaleFactors; proj_mode: RFE_PROJ_INVZ (:1596-1601, u = fx * (x * (1 / z)) + cx)
 *   or RFE_PROJ_DIV (Pinhole::project, u = (fx * x) / z + cx); dist_mode: RFE_DIST_FLOAT (:1635-1664) or RFE_DIST_TRUNC (:2149-2177:
 *   `int dist`, every candidate distance truncated toward zero before the strict <, accepted when (float)best <= th_accept).
 *   q [Np,256] map-point descriptors, pw [Np,3] GetWorldPos, normal [Np,3] GetNormal, min_dist / max_dist [Np]
 *   Get{Min,Max}DistanceInvariance (0.8f * mfMinDistance, 1.2f * mfMaxDistance: the distance gate), scale_dist [Np] the BARE mfMaxDistance
 *   that MapPoint::PredictScale divides by the distance (src/MapPoint.cc:696) -- not max_dist: with the usual scale factor 1.2 that
 *   would predict one level too many --, valid [Np] or NULL = all 1 (!isBad() && !spAlreadyFound.count(pMP));
 *   f [Nf,256], kpts / kxy (exactly one), nf_dev as rfe_search_by_projection_dev; matched_in [Nf] or NULL (vpMatched[f] != NULL);
 *   th_accept: TH_LOW for the first overload, TH_LOW * ratioHamming for the second.
 *   matched [Nf]: the accepted map point of the feature, -1 = none (a pre-matched feature stays -1); best_idx / best_dist / second_dist
 *   [Np] as rfe_search_by_projection (truncated values in RFE_DIST_TRUNC); proj [Np,2], radius [Np], level [Np] (0, 0 / 0 / -1 for a
 *   rejected point); reject [Np]: 0 = searched, else the first gate that failed: 1 invalid, 2 z < 0, 3 outside the image, 4 distance
 *   outside [min_dist, max_dist], 5 viewing angle (all but matched may be NULL); stats [8]: 0..3 as rfe_search_by_projection, 4 = map
 *   points that reached the search, 5..7 = 0.
 * The _dev form takes DEVICE pointers and is asynchronous on the ctx stream (no host synchronisation, no host read of device data once
 * the workspace has its size; cand_cap and overflow as rfe_search_by_projection_dev; stats is required).  The host form sizes the slots
 * itself and returns stats[0] >= 0.
 * Refused (RFE_ERR_INVALID): Np outside 0..16384; Nf outside 0..4096; empty bounds; nlevels outside 1..RFE_MAX_LEVELS; log_scale_factor
 *   <= 0 when nlevels > 1; an unknown proj_mode / dist_mode; cand_cap < 0; both or neither of kpts / kxy; a NULL required pointer; host
 *   form only: a non-finite pose, intrinsic, bound, scale factor, log_scale_factor, th_accept or keypoint.  The per-point arrays (pw,
 *   normal, min_dist, max_dist, scale_dist) are not checked in either form: a NaN there fails a gate on the device (a NaN coordinate
 *   is "outside the image") or, behind the gates, gives level 0.
 * Out of scope: KannalaBrandt8 and two-camera keyframes (the caller keeps the reference's loop), both Fuse overloads. */
#define RFE_PROJ_INVZ 0
#define RFE_PROJ_DIV 1
#define RFE_DIST_FLOAT 0
#define RFE_DIST_TRUNC 1
typedef struct rfe_sim3_params {
    float quat[4];                 /* x, y, z, w */
    float t[3];
    float ow[3];
    float fx, fy, cx, cy;
    float min_x, min_y, max_x, max_y;
    int32_t th;
    int32_t nlevels;
    float log_scale_factor;
    float scale_factors[RFE_MAX_LEVELS];
    int32_t proj_mode, dist_mode;
} rfe_sim3_params;
int rfe_search_by_projection_sim3_dev(rfe_ctx* ctx, const rfe_sim3_params* params, const float* q_dev, const float* pw_dev,
                                      const float* normal_dev, const float* min_dist_dev, const float* max_dist_dev,
                                      const float* scale_dist_dev, const uint8_t* valid_dev, int Np, const float* f_dev, const float* kpts_dev, const int32_t* kxy_dev,
                                      const uint8_t* matched_in_dev, int Nf, const int32_t* nf_dev, float th_accept, int cand_cap,
                                      int32_t* matched_dev, int32_t* best_idx_dev, float* best_dist_dev, float* second_dist_dev,
                                      float* proj_dev, float* radius_dev, int32_t* level_dev, int32_t* reject_dev, int32_t* stats_dev);
int rfe_search_by_projection_sim3(rfe_ctx* ctx, const rfe_sim3_params* params, const float* q, const float* pw, const float* normal,
                                  const float* min_dist, const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np,
                                  const float* f,
                                  const float* kpts, const int32_t* kxy, const uint8_t* matched_in, int Nf, float th_accept,
                                  int32_t* matched, int32_t* best_idx, float* best_dist, float* second_dist, float* proj, float* radius,
                                  int32_t* level, int32_t* reject, int32_t* stats);

/* ---- steps 2 and 3 of Tracking::SearchLocalPoints as one call ----
 * Frame::isInFrustum(pMP, 0.5) for every local map point (src/Tracking.cc:4124-4147, src/Frame.cc:711-794, one pinhole camera) and
 * SPmatcher::SearchByProjection1 over the points that passed (src/Matchers/SPmatcher.cc:1178-1283): the front (transform, projection, the
 * gates, MapPoint::PredictScale, RadiusByViewingCos, the far-point gate) in one kernel, then the grid, candidate lists, scan and sequential
 * assignment of rfe_search_by_projection, unchanged.  All arithmetic is fp32 in this order, one rounding per operation, no contraction:
 *   x = ((r00 px + r01 py) + r02 pz) + tx (y, z alike; rcw row-major), depth = sqrtf((x x + y y) + z z), invz = 1 / z;
 *   u = (fx x) / z + cx, v = (fy y) / z + cy; PO = P - ow, dist = sqrtf((POx POx + POy POy) + POz POz);
 *   viewCos = ((POx nx + POy ny) + POz nz) / dist; predicted level = ceilf(logf(scale_dist / dist) / log_scale_factor) clamped as a float to
 *   0..nlevels-1 (NaN = 0); radius = ((viewCos > 0.998 (the double literal) ? 2.5f : 4.0f) * th) * scale_factors[L].
 * reject [Np], the first gate that failed: 1 = invalid, 2 = z < 0 (z == +-0 passes), 3 = u < min_x || u > max_x || v < min_y || v > max_y
 *   (closed: u == max_x passes; a NaN u or v passes too, as in the reference, and is searched with an empty candidate list), 4 = dist <
 *   min_dist || dist > max_dist, 5 = viewCos < view_cos_limit, 6 = in the frustum but far_points && depth > th_far (not searched),
 *   0 = searched.
 *   rfe_frustum_params: rcw = mRcw (row-major), tcw = mtcw, ow = mOw; fx, fy, cx, cy, mbf; the frame's mnMinX, mnMinY, mnMaxX, mnMaxY;
 *   view_cos_limit (0.5 in SearchLocalPoints); th (a float in SearchByProjection1); far_points / th_far = bFarPoints / thFarPoints;
 *   nlevels = mnScaleLevels (1..RFE_MAX_LEVELS), log_scale_factor = mfLogScaleFactor, scale_factors = mvScaleFactors; level_mode:
 *   RFE_LEVEL_ZERO (the reference as written, :1193 nPredictedLevel = 0: L = 0 and the octave gate of the search is that of level 0) or
 *   RFE_LEVEL_PREDICTED (ORB-SLAM3's form: L = the predicted level, which is also the pred_level of the search).
 *   q [Np,256], pw [Np,3] GetWorldPos, normal [Np,3] GetNormal, min_dist / max_dist [Np] Get{Min,Max}DistanceInvariance, scale_dist [Np] the
 *   bare mfMaxDistance (as rfe_search_by_projection_sim3), valid [Np] or NULL = all 1 (mnLastFrameSeen != F.mnId && !isBad()), observed [Np]
 *   or NULL = all 1; f, kpts / kxy (exactly one), octave, skip, Nf, nf_dev, th_high, cand_cap, assign, best_idx, best_dist, second_dist and
 *   stats[0..3] exactly as rfe_search_by_projection[_dev].
 *   What isInFrustum leaves in the map point, per reject code (each array may be NULL):
 *     proj [Np,2] = (mTrackProjX, mTrackProjY): (0, 0) for 1, (-1, -1) for 2 and 3, (u, v) for 4, 5, 6 and 0;
 *     proj_xr [Np] = u - mbf * invz, depth [Np] = mTrackDepth, view_cos [Np]: for 0 and 6, else 0;
 *     level [Np] = mnTrackScaleLevel, the PREDICTED level in both level modes: for 0 and 6, else -1.
 *   stats [8]: 0..3 as rfe_search_by_projection, 4 = points in the frustum (codes 0 and 6: the reference's nToMatch, the IncreaseVisible
 *   calls), 5 = points searched (code 0), 6..7 = 0.
 * The _dev form takes DEVICE pointers and is asynchronous on the ctx stream (no host synchronisation, no host read of device data once
 * the workspace has its size; cand_cap and overflow as rfe_search_by_projection_dev -- the front's outputs and stats[4..5] do not depend
 * on the slots; stats is required).  The host form sizes the slots itself and returns stats[0] >= 0.
 * Refused (RFE_ERR_INVALID): Np outside 0..16384; Nf outside 0..4096; empty bounds; nlevels outside 1..RFE_MAX_LEVELS; log_scale_factor
 *   <= 0 when nlevels > 1; an unknown level_mode; cand_cap < 0; both or neither of kpts / kxy; a NULL required pointer; host form only: a
 *   non-finite pose, intrinsic, bound, th, th_high, view_cos_limit, th_far, scale factor, log_scale_factor or keypoint.  The per-point
 *   arrays are not checked in either form.
 * Out of scope: two-camera frames (Nleft != -1: isInFrustumChecks and the right-camera branch) and KannalaBrandt8 -- the caller keeps the
 * reference's loops. */
#define RFE_LEVEL_ZERO 0
#define RFE_LEVEL_PREDICTED 1
typedef struct rfe_frustum_params {
    float rcw[9];                  /* row-major */
    float tcw[3];
    float ow[3];
    float fx, fy, cx, cy, mbf;
    float min_x, min_y, max_x, max_y;
    float view_cos_limit;
    float th;
    int32_t far_points;
    float th_far;
    int32_t nlevels;
    float log_scale_factor;
    float scale_factors[RFE_MAX_LEVELS];
    int32_t level_mode;
} rfe_frustum_params;
int rfe_search_local_points_dev(rfe_ctx* ctx, const rfe_frustum_params* params, const float* q_dev, const float* pw_dev,
                                const float* normal_dev, const float* min_dist_dev, const float* max_dist_dev, const float* scale_dist_dev,
                                const uint8_t* valid_dev, const uint8_t* observed_dev, int Np, const float* f_dev, const float* kpts_dev,
                                const int32_t* kxy_dev, const int32_t* octave_dev, const uint8_t* skip_dev, int Nf, const int32_t* nf_dev,
                                float th_high, int cand_cap, int32_t* assign_dev, int32_t* best_idx_dev, float* best_dist_dev,
                                float* second_dist_dev, float* proj_dev, float* proj_xr_dev, float* depth_dev, float* view_cos_dev,
                                int32_t* level_dev, int32_t* reject_dev, int32_t* stats_dev);
int rfe_search_local_points(rfe_ctx* ctx, const rfe_frustum_params* params, const float* q, const float* pw, const float* normal,
                            const float* min_dist, const float* max_dist, const float* scale_dist, const uint8_t* valid,
                            const uint8_t* observed, int Np, const float* f, const float* kpts, const int32_t* kxy, const int32_t* octave,
                            const uint8_t* skip, int Nf, float th_high, int32_t* assign, int32_t* best_idx, float* best_dist,
                            float* second_dist, float* proj, float* proj_xr, float* depth, float* view_cos, int32_t* level, int32_t* reject,
                            int32_t* stats);

/* ---- LocalMapping::CreateNewMapPoints behind the matcher, for all neighbours in one call ----
 * The filter of SPmatcher::SearchForTriangulation (src/Matchers/SPmatcher.cc:1376-1393) and the geometry loop of
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:662-943) over the matches rfe_match_dev left on the device for P = Nn pairs
 * (current keyframe, neighbour n): S [Nn] and pairs [Nn,Kmax,2] exactly as it writes them, side 0 the current keyframe, i ascending, every
 * i and every j at most once per neighbour.  One pinhole camera per keyframe (NLeft == -1, no mpCamera2), mono and rectified stereo /
 * RGB-D.  The neighbours must be DISTINCT keyframes (has_mp2 of neighbour n is never changed by another neighbour).
 *   rfe_tri_params: inertial = mbInertial (parallax bound 0.9996, else 0.9998); far_points / th_far = mbFarPoints / mThFarPoints;
 *   ratio_factor = 1.5f * mfScaleFactor; nlevels (1..RFE_MAX_LEVELS), scale_factors = mvScaleFactors, level_sigma2 = mvLevelSigma2: ONE
 *   set for the whole call -- all keyframes of a map come from one extractor.  An octave outside 0..RFE_MAX_LEVELS-1 reads level 0.
 *   rfe_tri_view: rcw (row-major), tcw = GetPose(), ow = GetCameraCenter(); fx, fy, cx, cy, invfx, invfy, mb, mbf of the keyframe.
 *   view1 (HOST pointer in both forms) and kpts1 [N1,2] = mvKeysUn, kpts1_raw [N1,2] = mvKeys or NULL = kpts1 (KeyFrame::UnprojectStereo
 *   reads mvKeys), octave1, uright1 = mvuRight, depth1 = mvDepth, has_mp1 [N1] u8 = GetMapPoint(i) != NULL; per neighbour views2 [Nn],
 *   kpts2 / kpts2_raw [Nn,N2max,2], octave2, uright2, depth2, has_mp2 [Nn,N2max], n2 [Nn] (features of neighbour n, <= N2max),
 *   neighbour_valid [Nn] u8 or NULL = all 1: the baseline test of :600-620, which the caller makes (ComputeSceneMedianDepth included).
 * Per slot (n, k < S[n]) the statements run in the reference's order; code [Nn,Kmax] is the first `continue` taken:
 *    0 created                      1 neighbour skipped (neighbour_valid)   2 i outside 0..N1-1 or j outside 0..n2[n]-1 (nothing is read)
 *    3 existing map point (has_mp1[i] || has_mp2[n,j])                      4 Triangulate: x3Dh.w == 0 (:797)
 *    5 no stereo and low parallax (:815)    6 UnprojectStereo: depth <= 0 (:823)    7 z1 <= 0    8 z2 <= 0
 *    9 / 10 reprojection in view 1, mono (5.991) / stereo (7.8)            11 / 12 the same in view 2
 *   13 dist1 == 0 || dist2 == 0    14 far point    15 scale consistency    16 passed every gate, claimed by an earlier neighbour
 *   -1 for k >= S[n] (S[n] is clamped to 0..Kmax).
 * fp32, one rounding per operation, no contraction, plain / and sqrtf; dot and norm as ((a0 b0 + a1 b1) + a2 b2) and sqrtf of it:
 *   xn = ((kp.x - cx) / fx, (kp.y - cy) / fy, 1); ray = Rcw^T xn, ray[a] = (r0a xn.x + r1a xn.y) + r2a;
 *   cosParallaxRays = dot(ray1, ray2) / (norm(ray1) * norm(ray2)); z1 = ((r20 X + r21 Y) + r22 Z) + tz, x1 and y1 alike;
 *   mono: ((fx x1) / z1 + cx) - kp.x (Pinhole::project); stereo: u = (fx x1) invz + cx, u_r = u - mbf invz, three-term sum left to right;
 *   UnprojectStereo: x = ((u - cx) z) invfx, y alike, x3D[a] = ((r0a x + r1a y) + r2a z) + ow[a];
 *   dist = norm(x3D - ow); ratioDist = dist2 / dist1; ratioOctave = scale_factors[octave1] / scale_factors[octave2].
 *   In double, as the reference writes them: invz = (float)(1.0 / z); err > 5.991 * sigma2 and err > 7.8 * sigma2 (double products);
 *   cosParallaxRays < 0.9998 / < 0.9996 against the double literals (as float comparisons: < 0x1.ffe5cap-1f / < 0x1.ffcb94p-1f).
 * Reproduced as written: `else if (bStereo2)` -- the neighbour's stereo parallax is only computed when the current keyframe's feature is
 *   not stereo (:767-775); u2_r uses the CURRENT keyframe's mbf (:886); UnprojectStereo tests z > 0 again; a NaN passes every < / > gate,
 *   so a NaN point can be created (stats[5] counts them: drop them if you must); bOnlyStereo and bCoarse change nothing.
 * Two departures, which ARE this contract (the reference's own build may round differently):
 *   (a) the stereo parallax cos(2 atan2(mb / 2, depth)) is (d d - h h) / (d d + h h), h = mb / 2, in fp32;
 *   (b) Triangulate: A as at GeometricTools.cc:73-76; the null vector by a one-sided (Hestenes) Jacobi iteration on the columns of A that
 *       accumulates V: 6 sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); per pair alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q
 *       as left-associated 4-term sums; no rotation when gamma == 0, else zeta = (beta - alpha) / (2 gamma), t = (zeta >= 0 ? 1 : -1) /
 *       (|zeta| + sqrtf(1 + zeta zeta)), c = 1 / sqrtf(1 + t t), s = c t, (a_p, a_q) <- (c a_p - s a_q, s a_p + c a_q), V alike; x3Dh = the
 *       column of V whose column of A has the smallest squared norm (the first minimum); w == 0 fails the slot, else x3D = xyz / w.
 * Across neighbours: the reference adds the point to the current keyframe at once (:930), so a later neighbour skips that feature --
 *   for every i the slot of the LOWEST n that passes every gate creates the point, the other passing slots get code 16.
 * Outputs (device pointers in the _dev form; every one but stats may be NULL): code [Nn,Kmax]; x3d [Nn,Kmax,3], the point of every slot
 *   that got as far as the depth tests (codes 0 and 7..16), else 0; point_stereo [Nn,Kmax] u8 = bPointStereo (1 for code 6 too); the
 *   points created in creation order (n ascending, then k): out_n, out_idx1, out_idx2 (i32), out_x3d [.,3], out_stereo (u8), each with
 *   room for N1 entries (a feature is created once; entries past N1, which only input outside the contract can cause, are not written);
 *   matches [Nn] = S[n] for a valid neighbour, else 0 (their sum is the reference's matchsum).
 *   stats [8]: 0 points created, 1 slots examined (the S[n] of valid neighbours), 2 slots dropped for an existing map point (code 3),
 *   3 countStereo, 4 countStereoAttempt (slots whose feature an earlier neighbour took are not counted: the reference never sees them),
 *   5 created points with a non-finite coordinate, 6..7 = 0.
 * The _dev form is asynchronous on the ctx stream: no host synchronisation and no host read of device data once the workspace has its
 * size.  The host form stages its arrays and returns stats[0] >= 0.
 * Refused (RFE_ERR_INVALID): Nn outside 0..64; N1, N2max or Kmax outside 0..4096; nlevels outside 1..RFE_MAX_LEVELS; a NULL required
 *   pointer; host form only: a non-finite pose, intrinsic, mb, mbf, th_far, ratio_factor, scale factor or sigma2.  The per-feature arrays
 *   are not checked in either form.
 * Out of scope: KannalaBrandt8 and two-camera rigs -- the caller keeps the reference's loop. */
typedef struct rfe_tri_params {
    int32_t inertial;
    int32_t far_points;
    float th_far;
    float ratio_factor;
    int32_t nlevels;
    float scale_factors[RFE_MAX_LEVELS];
    float level_sigma2[RFE_MAX_LEVELS];
} rfe_tri_params;
typedef struct rfe_tri_view {
    float rcw[9];                  /* row-major */
    float tcw[3];
    float ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
} rfe_tri_view;
int rfe_triangulate_neighbours_dev(rfe_ctx* ctx, const rfe_tri_params* params, const rfe_tri_view* view1, const float* kpts1_dev,
                                   const float* kpts1_raw_dev, const int32_t* octave1_dev, const float* uright1_dev, const float* depth1_dev,
                                   const uint8_t* has_mp1_dev, int N1, const rfe_tri_view* views2_dev, const float* kpts2_dev,
                                   const float* kpts2_raw_dev, const int32_t* octave2_dev, const float* uright2_dev, const float* depth2_dev,
                                   const uint8_t* has_mp2_dev, const int32_t* n2_dev, const uint8_t* neighbour_valid_dev, int Nn, int N2max,
                                   const int32_t* S_dev, const int32_t* pairs_dev, int Kmax, int32_t* code_dev, float* x3d_dev,
                                   uint8_t* point_stereo_dev, int32_t* out_n_dev, int32_t* out_idx1_dev, int32_t* out_idx2_dev,
                                   float* out_x3d_dev, uint8_t* out_stereo_dev, int32_t* matches_dev, int32_t* stats_dev);
int rfe_triangulate_neighbours(rfe_ctx* ctx, const rfe_tri_params* params, const rfe_tri_view* view1, const float* kpts1,
                               const float* kpts1_raw, const int32_t* octave1, const float* uright1, const float* depth1,
                               const uint8_t* has_mp1, int N1, const rfe_tri_view* views2, const float* kpts2, const float* kpts2_raw,
                               const int32_t* octave2, const float* uright2, const float* depth2, const uint8_t* has_mp2, const int32_t* n2,
                               const uint8_t* neighbour_valid, int Nn, int N2max, const int32_t* S, const int32_t* pairs, int Kmax,
                               int32_t* code, float* x3d, uint8_t* point_stereo, int32_t* out_n, int32_t* out_idx1, int32_t* out_idx2,
                               float* out_x3d, uint8_t* out_stereo, int32_t* matches, int32_t* stats);

/* ---- Optimizer::PoseOptimization on the device: motion-only Levenberg-Marquardt on matched points ----
 * src/Optimizer.cc:55-401 over g2o's OptimizationAlgorithmLevenberg, one SE3 vertex and one unary edge per feature with a map point: B
 * problems per call, one workgroup each, the four rounds, their LM iterations and the chi2 re-classification between them inside the
 * kernel.  Double precision throughout; every sum over edges in one fixed order, so the outputs equal the restatement
 * tests/pose_opt_ref.py bit for bit (6i states the arithmetic and its three departures from the reference's own build).
 * Per problem, of N rows the first n (n_dev, clamped to 0..N; NULL = N) are features:
 *   pose0 [7]      the frame's Tcw as qx qy qz qw tx ty tz (floats), the start of EVERY round
 *   kpts_un [N,2]  mvKeysUn[i].pt;  octave [N] (NULL = 0; outside 0..nlevels-1 reads level 0);  uright [N] mvuRight (NULL = all mono; < 0:
 *                  a mono edge, otherwise stereo);  xw [N,3] the map point's GetWorldPos();  has_mp [N] != 0: mvpMapPoints[i] != NULL
 * params: fx, fy, cx, cy, bf = mbf; inv_level_sigma2 = mvInvLevelSigma2; iterations per round (0 = the reference's 10) and max_trials
 *   (0 = g2o's 10).
 * Outputs: pose [7] doubles, the estimate after the last round (pose0 widened when fewer than 3 edges: the reference returns before
 *   SetPose); pose_f32 its plain cast, which a later call can take as pose0; outlier [N] = mvbOutlier, written where has_mp is set among
 *   the n features and left alone elsewhere; chi2 [N] the float chi2 the last classification compared, written like outlier once a round
 *   has run; trace [4,8] per round: LM iterations, trials, the final lambda, the final currentChi, inliers after the round, 0, 0, 0 (rows of
 *   rounds not run are 0); stats [8]: 0 the return value nInitialCorrespondences - nBad (0 below three edges), 1 nInitialCorrespondences,
 *   2 nBad, 3 rounds run, 4 LM iterations, 5 trials, 6 rejected trials, 7 flags: 1 a round ended on a rejected trial (its classification
 *   used the errors of the rejected estimate, as the reference's does), 2 a solve found the system not positive, 4 a trial estimate or the
 *   final pose was not finite.
 * The _dev form is asynchronous on the ctx stream: no host synchronisation, no host read of device data, no workspace.  The host form
 * stages its arrays (outlier and chi2 go in and out) and returns stats[0] of problem 0 (0 when B = 0).
 * Refused (RFE_ERR_INVALID): B outside 0..64; N outside 0..4096; nlevels outside 1..RFE_MAX_LEVELS; a negative iterations[] or
 *   max_trials; a NULL required pointer (params, pose0, pose, outlier, stats; kpts_un, xw, has_mp when B N > 0); host form only: a
 *   non-finite fx, fy, cx, cy, bf, inv_level_sigma2 or pose0.  The per-feature arrays are not checked: a NaN world position runs through
 *   as in the reference and raises flag 4.
 * Out of scope: two-camera rigs (mpCamera2, EdgeSE3ProjectXYZOnlyPoseToBody) and KannalaBrandt8 -- the caller keeps the reference's
 *   function for those.  The inertial variants (PoseInertialOptimization*) are rfe_pose_inertial_optimization, below. */
typedef struct rfe_pose_params {
    float fx, fy, cx, cy, bf;
    int32_t nlevels;                          /* 1..RFE_MAX_LEVELS */
    float inv_level_sigma2[RFE_MAX_LEVELS];   /* mvInvLevelSigma2 */
    int32_t iterations[4];                    /* 0 = the reference's 10 */
    int32_t max_trials;                       /* 0 = g2o's 10 */
} rfe_pose_params;
int rfe_pose_optimization_dev(rfe_ctx* ctx, const rfe_pose_params* params, const float* pose0_dev, const float* kpts_un_dev,
                              const int32_t* octave_dev, const float* uright_dev, const float* xw_dev, const uint8_t* has_mp_dev,
                              const int32_t* n_dev, int B, int N, double* pose_dev, float* pose_f32_dev, uint8_t* outlier_dev, float* chi2_dev,
                              double* trace_dev, int32_t* stats_dev);
int rfe_pose_optimization(rfe_ctx* ctx, const rfe_pose_params* params, const float* pose0, const float* kpts_un, const int32_t* octave,
                          const float* uright, const float* xw, const uint8_t* has_mp, const int32_t* n, int B, int N, double* pose,
                          float* pose_f32, uint8_t* outlier, float* chi2, double* trace, int32_t* stats);

/* ---- Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame on the device: visual-inertial Gauss-Newton ----
 * src/Optimizer.cc:416-968 and :983-1623 with Marginalize (:1644-1725) over g2o's OptimizationAlgorithmGaussNewton and LinearSolverDense:
 * B problems per call, one workgroup each; the four rounds of ten Gauss-Newton iterations, the float chi2 classification between them,
 * the recovery pass, the final Hessian, the marginalisation of the previous frame and ConstraintPoseImu's eigenvalue clipping all run
 * inside the kernel.  Double precision (the preintegration's bias correction in float, as ImuTypes.cc:377-427 has it); every sum in one
 * fixed order, so the outputs equal the restatement tests/pose_inertial_ref.py bit for bit (6p states the arithmetic and its departures
 * from the reference's own build).  Single pinhole camera.
 * Per problem, of N rows the first n (n_dev, clamped to 0..N; NULL = N) are features:
 *   mode           RFE_PIO_LAST_KEYFRAME: the previous state is fixed, 15 free dimensions, no prior edge;  RFE_PIO_LAST_FRAME: the previous
 *                  state is free, 30 dimensions, EdgePriorPoseImu under Huber 5 and Marginalize(H, 0, 14) at the end
 *   rec_init       bRecInit (NULL = 0): != 0 skips the recovery pass
 *   cam [36]       floats, row-major rotations: the frame's GetPose() as Rcw 9, tcw 3 (read until the first update, as ImuCamPose's
 *                  constructor does); mImuCalib.mTcb as Rcb 9, tcb 3; mImuCalib.mTbc as Rbc 9 (not read: Rbc = Rcb^T), tbc 3
 *   state [21], prev_state [21]   floats: Rwb 9, twb 3, velocity 3, gyro bias 3, accelerometer bias 3 of the frame and of mpLastKeyFrame /
 *                  mpPrevFrame -- what the vertex constructors cast
 *   preint [RFE_PIO_PREINT_FLOATS]   the preintegration EdgeInertial is built from (mpImuPreintegrated / mpImuPreintegratedFrame): dT, dR 9,
 *                  dV 3, dP 3, JRg 9, JVg 9, JVa 9, JPg 9, JPa 9, its bias b as bax bay baz bwx bwy bwz, C's leading 9 x 9 block
 *   cov_rw [18]    C(9..11, 9..11) and C(12..14, 12..14) of mpImuPreintegrated, which InfoG / InfoA invert (LastFrame takes them from a
 *                  different preintegration than the edge, :1213 against :1233, :1246; the two arrays let the caller reproduce that)
 *   prior_in [RFE_PIO_PRIOR_DOUBLES]   LastFrame only: the previous frame's ConstraintPoseImu as doubles Rwb 9, twb 3, vwb 3, bg 3, ba 3, H 225
 *   kpts_un, octave, uright, xw, has_mp   as rfe_pose_optimization;  track_depth [N] the map point's mTrackDepth (bClose = < 10.f)
 * params: fx, fy, cx, cy, bf = mbf; inv_level_sigma2 = mvInvLevelSigma2.
 * Outputs: state_out [21] doubles, the optimised Rwb, twb, velocity, bg, ba; state_f32 their float casts (what SetImuPoseVelocity and
 *   IMU::Bias receive), which a later call takes as prev_state; outlier [N] and chi2 [N] written where has_mp is set among the n features
 *   (chi2: the float the last classification or the recovery pass compared); prior_out [RFE_PIO_PRIOR_DOUBLES]: the state and the 15 x 15 H
 *   after ConstraintPoseImu's constructor, in prior_in's layout, so frame k's prior_out_dev is frame k + 1's prior_in_dev without leaving
 *   the device; trace [4,8] per round: iterations run, the active robust chi2 the first and the last iteration saw, 1 if every solve
 *   succeeded, inliers after the round, 0, 0, 0; stats [16]: 0 the return value nInitialCorrespondences - nBad, 1 nInitialCorrespondences,
 *   2 nBad, 3 mono edges, 4 stereo edges, 5 rounds run, 6 iterations run, 7 failed solves, 8 flags, 9 nInliers of the last round, 10..15 0.
 *   flags: 1 a solve found the system not positive (the stale x was applied and the round ended), 2 a non-finite output, 4 fewer than
 *   10 edges ended the rounds after the first, 8 the recovery pass ran, 16 an eigenvalue of EdgeInertial's information was clipped,
 *   32 the marginalisation cut a singular value, 64 an eigenvalue of prior_out's H was clipped, 128 the prior's Huber weight was below 1.
 *   256 (the _dev form only, which reads mode on the device and so cannot refuse it) the problem ran as LastKeyFrame because its mode was
 *   neither value or because it was LastFrame and prior_in_dev was NULL.
 * The _dev form is asynchronous on the ctx stream: no host synchronisation, no host read of device data, no workspace.  The host
 *   form stages its arrays (outlier and chi2 go in and out) and returns stats[0] of problem 0 (0 when B = 0).
 * Refused (RFE_ERR_INVALID), nothing written: B outside 0..64; N outside 0..4096; nlevels outside 1..RFE_MAX_LEVELS; a NULL required
 *   pointer (params, mode, cam, state, prev_state, preint, cov_rw, state_out, outlier, stats; kpts_un, xw, has_mp, track_depth when
 *   B N > 0); host form only: a mode that is neither value, LastFrame without prior_in, a dT that is not positive.
 * Out of scope: two-camera rigs (mpCamera2), KannalaBrandt8. */
enum { RFE_PIO_LAST_KEYFRAME = 0, RFE_PIO_LAST_FRAME = 1 };
#define RFE_PIO_CAM_FLOATS 36
#define RFE_PIO_STATE_FLOATS 21
#define RFE_PIO_PREINT_FLOATS 148
#define RFE_PIO_COV_RW_FLOATS 18
#define RFE_PIO_PRIOR_DOUBLES 246
typedef struct rfe_pose_inertial_params {
    float fx, fy, cx, cy, bf;
    int32_t nlevels;                          /* 1..RFE_MAX_LEVELS */
    float inv_level_sigma2[RFE_MAX_LEVELS];   /* mvInvLevelSigma2 */
} rfe_pose_inertial_params;
int rfe_pose_inertial_optimization_dev(rfe_ctx* ctx, const rfe_pose_inertial_params* params, const int32_t* mode_dev, const int32_t* rec_init_dev,
                                       const float* cam_dev, const float* state_dev, const float* prev_state_dev, const float* preint_dev,
                                       const float* cov_rw_dev, const double* prior_in_dev, const float* kpts_un_dev, const int32_t* octave_dev,
                                       const float* uright_dev, const float* xw_dev, const uint8_t* has_mp_dev, const float* track_depth_dev,
                                       const int32_t* n_dev, int B, int N, double* state_out_dev, float* state_f32_dev, uint8_t* outlier_dev,
                                       float* chi2_dev, double* prior_out_dev, double* trace_dev, int32_t* stats_dev);
int rfe_pose_inertial_optimization(rfe_ctx* ctx, const rfe_pose_inertial_params* params, const int32_t* mode, const int32_t* rec_init,
                                   const float* cam, const float* state, const float* prev_state, const float* preint, const float* cov_rw,
                                   const double* prior_in, const float* kpts_un, const int32_t* octave, const float* uright, const float* xw,
                                   const uint8_t* has_mp, const float* track_depth, const int32_t* n, int B, int N, double* state_out,
                                   float* state_f32, uint8_t* outlier, float* chi2, double* prior_out, double* trace, int32_t* stats);

/* ---- Sim3Solver on the device: every RANSAC hypothesis of a loop-closing candidate in one call ----
 * src/Sim3Solver.cc:61-483 as LoopClosing::DetectCommonRegionsFromBoW drives it (SetRansacParameters, then iterate(20, ..) until bConverge
 * or bNoMore): B problems per call, each with its own correspondences, poses, cameras, min_inliers and iteration count.  The front
 * (:61-121) takes both map points of every correspondence into their camera frames and images, one wave per hypothesis runs ComputeSim3
 * (:319-420, Horn's closed form) on its triple and counts the inliers of CheckInliers (:423-447), and one workgroup per problem makes the
 * reference's sequential choice: the FIRST hypothesis h < its whose count exceeds min_inliers (bConverge), otherwise the LAST hypothesis
 * that reaches the maximum count (bNoMore).  fp32, one rounding per operation, sums left to right; the outputs equal the restatement
 * tests/sim3_solver_ref.py bit for bit (6j states the arithmetic and its departures from the reference's own build: a fixed-schedule
 * Jacobi for Eigen's EigenSolver, the rotation straight from the unit quaternion, fixed evaluation orders, the random stream).
 * params [B] is a HOST array in both forms.  Per problem, of N rows the first n (clamped to 0..N) are correspondences and of H draws the
 * first its are used:
 *   params[b]      rcw1 / rcw2 row-major and tcw1 / tcw2: pKF1's and pKF2's pose; fx fy cx cy of each Pinhole camera; fix_scale;
 *                  min_inliers (mRansacMinInliers); its = mRansacMaxIts AFTER SetRansacParameters (rfe_sim3_ransac_iterations); n
 *   xw1, xw2 [N,3] GetWorldPos() of pMP1 and pMP2;  sigma2_1, sigma2_2 [N] mvLevelSigma2[octave] of the keypoint in pKF1 and in pKFm: the
 *                  bound of a side is (float)(uint64)(9.210 * (double)sigma2), mvnMaxError being a vector<size_t>
 *   draws [H,3]    the three RandomInt(0, size - 1) results of every iteration, resolved through the reference's swap-with-back list; a
 *                  draw outside 0..n-1-k is clamped and raises flag 8
 * Outputs per problem: T12 [16] row-major, R [9], t [3], s: mBestT12 / mBestRotation / mBestTranslation / mBestScale (the identity, 0 and 1
 *   when no hypothesis ran; NaN where the chosen triple's quaternion has a zero vector part, as the reference's 0 / 0 at :375 leaves them);
 *   inliers [N] the winner's mvbInliersi (all 0 without convergence, as vbInliers is; index it through mvnIndices1 yourself);
 *   best_inliers [N] mvbBestInliers; counts [H] mnInliersi of EVERY h < its (those behind the winner the reference would not have run);
 *   hyps [H,32] per hypothesis T12 [16], R [9], t [3], s, flags (int32 bits: 1 NaN rotation, 8 a clamped draw), 0, 0;
 *   stats [8]: 0 bConverge, 1 nInliers, 2 mnBestInliers, 3 the chosen hypothesis (-1: none ran), 4 mnIterations, 5 bNoMore, 6 hypotheses
 *   with a NaN rotation among the first mnIterations, 7 flags: 1 n < min_inliers, 2 n < 3 (the reference would draw from an empty list:
 *   handled as 1), 8 a clamped draw among the first its.  Rows behind n, entries behind its and rows of hyps behind its are left alone.
 * The _dev form is asynchronous on the ctx stream: no host synchronisation, no host read of device data, no allocation once the ctx's
 * workspace has the call's size; one front launch per 16 problems, one hypothesis launch, one selection launch.  The host form stages its
 * arrays and returns stats[0] of problem 0 (0 when B = 0).  inliers, best_inliers, counts, hyps, R, t and s may be NULL.
 * Refused (RFE_ERR_INVALID): B outside 0..64; N outside 0..4096; H outside 1..1024; its outside 1..H; min_inliers < 0; a NULL required
 *   pointer (params, draws, T12, stats; xw1, xw2, sigma2_1, sigma2_2 when B N > 0); host form only: a non-finite pose or intrinsic, a
 *   negative or non-finite sigma2 among the n rows.  Positions are not checked: a NaN runs through as an outlier.
 * rfe_sim3_ransac_iterations is SetRansacParameters' arithmetic (:137-147) on the host's libm: epsilon = (float)min_inliers / n, 1 when
 *   min_inliers == n, otherwise ceil(log(1 - probability) / log(1 - pow(epsilon, 3))), a quotient that is NaN or outside int converting
 *   to INT_MIN as on x86-64, then max(1, min(., max_its)).
 * Out of scope: KannalaBrandt8 cameras, the descriptor matching in front, a device-side random generator (OptimizeSim3: 6k, below). */
typedef struct rfe_sim3_solver_params {
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];   /* row-major */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    int32_t fix_scale, min_inliers, its, n;
} rfe_sim3_solver_params;
int rfe_sim3_ransac_dev(rfe_ctx* ctx, const rfe_sim3_solver_params* params, const float* xw1_dev, const float* xw2_dev,
                        const float* sigma2_1_dev, const float* sigma2_2_dev, const int32_t* draws_dev, int B, int N, int H, float* T12_dev,
                        float* R_dev, float* t_dev, float* s_dev, uint8_t* inliers_dev, uint8_t* best_inliers_dev, int32_t* counts_dev,
                        float* hyps_dev, int32_t* stats_dev);
int rfe_sim3_ransac(rfe_ctx* ctx, const rfe_sim3_solver_params* params, const float* xw1, const float* xw2, const float* sigma2_1,
                    const float* sigma2_2, const int32_t* draws, int B, int N, int H, float* T12, float* R, float* t, float* s,
                    uint8_t* inliers, uint8_t* best_inliers, int32_t* counts, float* hyps, int32_t* stats);
int rfe_sim3_ransac_iterations(double probability, int min_inliers, int n, int max_its);

/* ---- Optimizer::OptimizeSim3 on the device: the Sim3 refinement of a loop-closing candidate ----
 * src/Optimizer.cc:4195-4494 over g2o's OptimizationAlgorithmLevenberg: one free 7-DoF VertexSim3Expmap and, per matched map-point pair,
 * an EdgeSim3ProjectXYZ (pMP2 through S12 into KF1's image) and an EdgeInverseSim3ProjectXYZ (pMP1 through S12^-1 into KF2's), both
 * linearised by g2o's NUMERIC central differences (delta 1e-9).  B problems per call, one workgroup each; the robust round, the chi2
 * check, the plain round and the final classification run inside the kernel.  Double precision throughout; every sum over pairs in one
 * fixed order, so the outputs equal the restatement tests/optimize_sim3_ref.py bit for bit (6k states the arithmetic and its four
 * departures from the reference's own build).
 * params [B] is a HOST array in both forms.  Per problem, of N rows the first n (clamped to 0..N) are rows of vpMatches1 and of N2 rows
 * the first n2 are KF2's keypoints:
 *   params[b]      rcw1 / rcw2 row-major and tcw1 / tcw2: GetRotation() / GetTranslation() of pKF1 and pKF2; fx fy cx cy of each Pinhole
 *                  camera; nlevels and mvInvLevelSigma2 of each keyframe; th2; fix_scale; all_points; n; n2; iterations[3]: round 1, round 2
 *                  when round 1 removed no pair, round 2 otherwise (0 = the reference's 5, 5, 10); max_trials (0 = g2o's 10)
 *   s12_0 [8]      g2oS12 as qx qy qz qw tx ty tz s (doubles), taken as given: nothing is normalised
 *   xw1, xw2 [N,3] GetWorldPos() of pMP1 = pKF1's map point i and of pMP2 = vpMatches1[i];  valid [N] != 0: both exist and neither isBad()
 *   kpts1 [N,2]    pKF1->mvKeysUn[i].pt;  octave1 [N] its octave (NULL = 0; outside 0..nlevels1-1 reads level 0)
 *   idx2 [N]       get<0>(pMP2->GetIndexInKeyFrame(pKF2)): < 0 not in KF2 -- the row is skipped unless all_points, and observes the
 *                  NORMALISED float coordinates of pMP2 in KF2 at level 0, as the reference does (its own "BUG" comment, :4371-4382);
 *                  at or above n2: treated the same and flag 8
 *   kpts2 [N2,2], octave2 [N2]   pKF2->mvKeysUn[.].pt and octave (octave2 NULL = 0)
 * A row carries an edge pair iff valid, (all_points or idx2 >= 0) and not (z of pMP2 in KF2's frame < 0).
 * Outputs per problem: s12 [8] doubles, the estimate after round 2 -- the input when the return value is 0 through the early exit (:4457
 *   returns before g2oS12 is written); s12_f32 [8] its plain cast (the Sim3f the caller composes mScw from; rfe_search_by_projection_sim3 takes its transform in
 *   a HOST structure, so the chain into it costs one 32-byte read until that entry grows a device-side form); keep [N] in/out: cleared
 *   exactly where the reference nulls vpMatches1[i], every other byte left alone; chi2 [N,2] the doubles (e12, e21) the last
 *   classification of the row compared, rows without a pair left alone; trace [2,8] per round: LM iterations, trials, the final lambda,
 *   the final currentChi, surviving pairs, 0, 0, 0; stats [8]: 0 the return value (nIn, or 0), 1 nCorrespondences, 2 nBad, 3 rounds run,
 *   4 LM iterations, 5 trials, 6 rejected trials, 7 flags: 1 a round ended on a rejected trial (round 1's check then used the errors of
 *   the rejected estimate, as the reference's does), 2 a solve found the system not positive, 4 a trial or the final estimate was not
 *   finite, 8 an idx2 at or above n2, 16 the early exit (fewer than 10 pairs after round 1; with no pair at all no round runs).
 *   mAcumHessian is only ever zeroed by the reference (:4465): the device produces nothing for it.
 * The _dev form is asynchronous on the ctx stream: no host synchronisation, no host read of device data, no workspace; one launch per 8
 * problems.  The host form stages its arrays (keep and chi2 go in and out) and returns stats[0] of problem 0 (0 when B = 0).
 * s12_f32, chi2, trace, octave1, octave2 may be NULL; kpts2 when N2 = 0.
 * Refused (RFE_ERR_INVALID): B outside 0..64; N or N2 outside 0..4096; nlevels1 / nlevels2 outside 1..RFE_MAX_LEVELS; a negative
 *   iterations[] or max_trials; a NULL required pointer (params, s12_0, s12, keep, stats; xw1, xw2, valid, kpts1, idx2 when B N > 0; kpts2
 *   when B N2 > 0); host form only: a non-finite pose, intrinsic, inv_level_sigma2 or th2.  The per-row arrays are not checked: a NaN
 *   world position runs through as in the reference and raises flag 4.
 * Out of scope: KannalaBrandt8 and two-camera rigs, SearchByBoW in front, composing mScw = gScm gSmw, everything else in Optimizer. */
typedef struct rfe_optimize_sim3_params {
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];   /* row-major */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    int32_t nlevels1;                           /* 1..RFE_MAX_LEVELS */
    float inv_level_sigma2_1[RFE_MAX_LEVELS];   /* pKF1->mvInvLevelSigma2 */
    int32_t nlevels2;
    float inv_level_sigma2_2[RFE_MAX_LEVELS];   /* pKF2->mvInvLevelSigma2 */
    float th2;
    int32_t fix_scale, all_points, n, n2;
    int32_t iterations[3];                      /* 0 = the reference's 5, 5, 10 */
    int32_t max_trials;                         /* 0 = g2o's 10 */
} rfe_optimize_sim3_params;
int rfe_optimize_sim3_dev(rfe_ctx* ctx, const rfe_optimize_sim3_params* params, const double* s12_0_dev, const float* xw1_dev,
                          const float* xw2_dev, const uint8_t* valid_dev, const float* kpts1_dev, const int32_t* octave1_dev,
                          const int32_t* idx2_dev, const float* kpts2_dev, const int32_t* octave2_dev, int B, int N, int N2, double* s12_dev,
                          float* s12_f32_dev, uint8_t* keep_dev, double* chi2_dev, double* trace_dev, int32_t* stats_dev);
int rfe_optimize_sim3(rfe_ctx* ctx, const rfe_optimize_sim3_params* params, const double* s12_0, const float* xw1, const float* xw2,
                      const uint8_t* valid, const float* kpts1, const int32_t* octave1, const int32_t* idx2, const float* kpts2,
                      const int32_t* octave2, int B, int N, int N2, double* s12, float* s12_f32, uint8_t* keep, double* chi2, double* trace,
                      int32_t* stats);

/* ---- Optimizer::LocalBundleAdjustment on the device: the local-mapping thread's Schur-complement LM ----
 * src/Optimizer.cc:1857-2150 over g2o's BlockSolver_6_3 and OptimizationAlgorithmLevenberg: P free and F fixed SE3 keyframe vertices, L
 * marginalised 3-DoF point vertices, one mono (EdgeSE3ProjectXYZ) or stereo (EdgeStereoSE3ProjectXYZ) Huber edge per observation, ONE
 * robust optimize(iterations) and one classification.  One problem per call.  Double precision throughout; every sum in one fixed order,
 * so the outputs equal the restatement tests/local_ba_ref.py bit for bit (6l states the arithmetic and its departures from the
 * reference's own build, among them a dense unpivoted LDLT for the reduced pose system).
 *   K = P + F keyframes, the P free ones first in ascending mnId (g2o's Hessian order), then the fixed ones (the map's init keyframe
 *   goes with the fixed ones):  kf_pose [K,7] qx qy qz qw tx ty tz of GetPose() (widened and normalised as 6i);  kf_cam [K,5] fx fy cx cy
 *   mbf;  kf_nlevels [K] and kf_inv_level_sigma2 [K, RFE_MAX_LEVELS] (mvInvLevelSigma2);  kf_feat_off [K + 1]: keyframe k's features are
 *   rows kf_feat_off[k] .. kf_feat_off[k + 1] - 1 of kpts_un [Nf,2] (mvKeysUn[.].pt), octave [Nf] (NULL = 0; outside 0..nlevels-1 reads
 *   level 0) and uright [Nf] (mvuRight; NULL = all mono)
 *   xw [L,3]: GetWorldPos() of the local map points in ascending mnId
 *   edge_point / edge_kf / edge_feat [E]: one row per observation, point index, keyframe index, feature index INSIDE that keyframe; sorted
 *   by (point, keyframe) strictly ascending.  uright < 0: a mono edge; otherwise (NaN too) stereo
 * Outputs: pose [P,7] doubles and pose_f32 their cast (the free keyframes); point [L,3] and point_f32; erase [E] = chi2 > th2 ||
 *   !isDepthPositive, where chi2 [E] is the value the last computeActiveErrors left on the edge (stale after a run that ends on a
 *   rejected trial: flag 1) and the depth is taken at the final estimates; trace [iterations,4] per LM iteration run: trials, the lambda it
 *   left, currentChi, 0 (rows of iterations not run are zero); stats [8]: 0 LM iterations, 1 trials, 2 rejected trials, 3 failed solves,
 *   4 edges erased, 5 flags, 6 edges on free keyframes, 7 Schur pair-list entries.  Flags: 1 ended on a rejected trial, 2 a solve met a
 *   zero or non-finite pivot, 4 a trial or the final estimate was not finite, 8 *stop was seen set, 16 no LM iteration ran (iterations
 *   = 0 or stop preset): the reference would classify errors nobody computed; this entry evaluates them at the input estimate.
 * BOTH forms are synchronous: the LM loop runs on the host, one plain launch per stage on the ctx stream and one small pinned read per
 * trial, and `stop` (a HOST pointer, pbStopFlag, may be NULL) is read where g2o's terminate() is: before each iteration and after each
 * trial.  rfe_local_ba_dev keeps every array on the device but returns only when the optimisation has finished -- the one _dev entry
 * that is not asynchronous.  It validates the edge and keyframe tables in its first kernel and reads the verdict before anything else is
 * launched, so a bad index is a refusal, never a stray access.  Both return the number of erased edges (>= 0).
 * pose_f32, point_f32, chi2, trace, octave, uright may be NULL.
 * Refused (RFE_ERR_INVALID): P outside 0..RFE_LBA_MAX_FREE, K = P + F outside 1..RFE_LBA_MAX_KF, L outside 0..RFE_LBA_MAX_POINTS, E outside
 *   0..RFE_LBA_MAX_EDGES, Nf < 0; iterations outside 0..RFE_LBA_MAX_ITERATIONS, max_trials < 0; a non-finite th2 or user_lambda_init; a NULL
 *   required pointer; an nlevels outside 1..RFE_MAX_LEVELS; a kf_feat_off that decreases or leaves 0..Nf; an edge index out of range;
 *   edges not strictly ascending in (point, keyframe).  Nothing is written then.  The poses, positions and observations are not
 *   checked: a NaN world position runs through as in the reference and raises flags 2 and 4.
 * Out of scope: LocalInertialBA, the merge overload, global BundleAdjustment, EdgeSE3ProjectXYZToBody (two-camera rigs), KannalaBrandt8. */
#define RFE_LBA_MAX_FREE 64
#define RFE_LBA_MAX_KF 256
#define RFE_LBA_MAX_POINTS 16384
#define RFE_LBA_MAX_EDGES 131072
#define RFE_LBA_MAX_ITERATIONS 64
#define RFE_LBA_FLAG_ENDED_REJECTED 1
#define RFE_LBA_FLAG_SOLVE_FAILED 2
#define RFE_LBA_FLAG_NONFINITE 4
#define RFE_LBA_FLAG_STOPPED 8
#define RFE_LBA_FLAG_NO_ITERATION 16
typedef struct rfe_local_ba_params {
    int32_t iterations;          /* optimizer.optimize(10); 0 runs none */
    int32_t max_trials;          /* 0 = g2o's 10 */
    double user_lambda_init;     /* 0, or 100 for pMap->IsInertial() */
    double th2_mono, th2_stereo; /* 5.991, 7.815: the classification compares doubles; the Huber deltas are (float) sqrt of them */
    const volatile uint8_t* stop;/* HOST pointer or NULL: pbStopFlag */
} rfe_local_ba_params;
int rfe_local_ba_dev(rfe_ctx* ctx, rfe_local_ba_params params, const float* kf_pose_dev, const float* kf_cam_dev, const int32_t* kf_nlevels_dev,
                     const float* kf_inv_level_sigma2_dev, const int32_t* kf_feat_off_dev, const float* kpts_un_dev, const int32_t* octave_dev,
                     const float* uright_dev, const float* xw_dev, const int32_t* edge_point_dev, const int32_t* edge_kf_dev,
                     const int32_t* edge_feat_dev, int P, int F, int L, int E, int Nf, double* pose_dev, float* pose_f32_dev, double* point_dev,
                     float* point_f32_dev, uint8_t* erase_dev, double* chi2_dev, double* trace_dev, int32_t* stats_dev);
int rfe_local_ba(rfe_ctx* ctx, rfe_local_ba_params params, const float* kf_pose, const float* kf_cam, const int32_t* kf_nlevels,
                 const float* kf_inv_level_sigma2, const int32_t* kf_feat_off, const float* kpts_un, const int32_t* octave, const float* uright,
                 const float* xw, const int32_t* edge_point, const int32_t* edge_kf, const int32_t* edge_feat, int P, int F, int L, int E, int Nf,
                 double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* erase, double* chi2, double* trace, int32_t* stats);

/* ---- Optimizer::OptimizeEssentialGraph on the device: the Sim3 pose graph that corrects the map after a loop ----
 * src/Optimizer.cc:4509-4840 over g2o's BlockSolver_7_3 and OptimizationAlgorithmLevenberg: one VertexSim3Expmap per keyframe, one
 * EdgeSim3 (identity information, no robust kernel, numeric Jacobians with delta 1e-9) per edge, optimize(iterations), then the poses
 * and the map points' correction.  One graph per call.  Double precision throughout; every sum in one fixed order, so the outputs equal
 * the restatement tests/essential_graph_ref.py bit for bit (6m states the arithmetic and its departures, among them a dense unpivoted
 * LDLT that the kernels run over 28 x 28 tiles, skipping the tiles the pattern can never fill).
 *   s_est [N,8] qx qy qz qw tx ty tz s: vScw, every keyframe's estimate (the CorrectedSim3 entry, or the SE3 pose at scale 1)
 *   s_meas [N,8]: the NonCorrectedSim3 entry where there is one, a copy of s_est otherwise
 *   fixed [N]: non-zero for mnId == GetInitKFid(); zero fixed vertices is accepted and runs
 *   edge_i / edge_j / edge_from_est [E]: vertex 0 and vertex 1 of every edge in ascending (i, j), duplicates kept, i != j; the
 *   measurement is Sji = Sjw Swi from s_est when edge_from_est is non-zero (loop connections), from s_meas otherwise
 *   xw [L,3] float and point_ref [L]: the map points and the keyframe each is corrected through, -1 for a point that is copied
 * Outputs: siw [N,8] the corrected Sim3; tiw_f32 [N,7] (float) q and (float) t / (float) s, what SetPose takes; swi [N,8] the inverses;
 *   xw_out [L,3] = Swr'.map(Srw.map(X)) in double, Srw the INPUT s_est of the reference keyframe, cast to float; chi2 [E] at the final
 *   estimate (the closing computeActiveErrors); trace [iterations,4] per LM iteration run: trials, the lambda it left, currentChi, 0;
 *   stats [8]: 0 LM iterations, 1 trials, 2 rejected trials, 3 failed solves, 4 flags, 5 free vertices, 6 tiles the factorisation
 *   processes, 7 tiles of the dense lower triangle.  Flags: 1 ended on a rejected trial, 2 a solve failed (a zero or non-finite pivot,
 *   a non-finite entry of L or of the solution), 4 a trial or the final estimate was not finite, 16 no LM iteration ran.
 * BOTH forms are synchronous, like rfe_local_ba: the LM loop runs on the host, plain launches on the ctx stream and one small pinned
 * read per linearisation and per trial.  The _dev form validates the edge table and point_ref in its first kernels and reads the
 * verdict before anything indexes by them.  Both return the number of LM iterations run (>= 0).
 * tiw_f32, swi, chi2, trace may be NULL.
 * Refused (RFE_ERR_INVALID): N outside 1..RFE_EG_MAX_KF, E outside 0..RFE_EG_MAX_EDGES, L outside 0..RFE_EG_MAX_POINTS, iterations
 *   outside 0..RFE_EG_MAX_ITERATIONS, max_trials < 0, a non-finite user_lambda_init, a NULL required pointer, an edge index out of
 *   range, an edge from a keyframe to itself, edges not ascending, a point_ref outside -1..N-1.  Nothing is written then.
 * Out of scope: OptimizeEssentialGraph4DoF, the merge overload, the inertial edges. */
#define RFE_EG_MAX_KF 1024
#define RFE_EG_MAX_EDGES 16384
#define RFE_EG_MAX_POINTS (1 << 20)
#define RFE_EG_MAX_ITERATIONS 64
#define RFE_EG_FLAG_ENDED_REJECTED 1
#define RFE_EG_FLAG_SOLVE_FAILED 2
#define RFE_EG_FLAG_NONFINITE 4
#define RFE_EG_FLAG_NO_ITERATION 16
typedef struct rfe_essential_graph_params {
    int32_t iterations;          /* optimizer.optimize(20); 0 runs none */
    int32_t max_trials;          /* 0 = g2o's 10 */
    double user_lambda_init;     /* setUserLambdaInit(1e-16); <= 0: g2o's 1e-5 max |diagonal| */
    int32_t fix_scale;           /* bFixScale */
    int32_t reserved;
} rfe_essential_graph_params;
int rfe_essential_graph_dev(rfe_ctx* ctx, rfe_essential_graph_params params, const double* s_est_dev, const double* s_meas_dev,
                            const uint8_t* fixed_dev, const int32_t* edge_i_dev, const int32_t* edge_j_dev, const uint8_t* edge_from_est_dev,
                            const float* xw_dev, const int32_t* point_ref_dev, int N, int E, int L, double* siw_dev, float* tiw_f32_dev,
                            double* swi_dev, float* xw_out_dev, double* chi2_dev, double* trace_dev, int32_t* stats_dev);
int rfe_essential_graph(rfe_ctx* ctx, rfe_essential_graph_params params, const double* s_est, const double* s_meas, const uint8_t* fixed,
                        const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_from_est, const float* xw, const int32_t* point_ref,
                        int N, int E, int L, double* siw, float* tiw_f32, double* swi, float* xw_out, double* chi2, double* trace,
                        int32_t* stats);

/* ---- Optimizer::GlobalBundleAdjustemnt on the device: the full bundle adjustment behind a loop closure ----
 * src/Optimizer.cc:2832-3220 (BundleAdjustment, reached from GlobalBundleAdjustemnt and from the monocular initialisation) over g2o's
 * BlockSolver_6_3 and OptimizationAlgorithmLevenberg: one SE3 vertex per keyframe, one marginalised 3-DoF vertex per map point, one mono
 * or stereo edge per observation, ONE optimize(iterations); no classification.  One problem per call.  It is rfe_local_ba's arithmetic up
 * to the reduced system (6l) behind a structure front whose work scales with the Schur pairs, and rfe_essential_graph's tiled LDLT (6m)
 * on 24 x 24 tiles over the fill of the covisibility pattern, so it runs past 64 free keyframes.  Double precision throughout; every sum
 * in one fixed order, so the outputs equal the restatement tests/global_ba_ref.py bit for bit.
 *   K keyframes in ascending mnId:  kf_pose [K,7] qx qy qz qw tx ty tz (the layout of rfe_essential_graph's tiw_f32; widened and normalised
 *   as 6i), kf_cam [K,5], kf_nlevels [K], kf_inv_level_sigma2 [K, RFE_MAX_LEVELS], kf_feat_off [K + 1] as rfe_local_ba;  fixed [K]: non-zero
 *   for mnId == GetInitKFid() -- none or several are accepted and run.  The free keyframes in ascending index are the Hessian order
 *   kpts_un [Nf,2], octave [Nf] (NULL = 0), uright [Nf] (NULL = all mono) as rfe_local_ba;  xw [L,3]: the map points in ascending mnId (the
 *   layout of rfe_essential_graph's xw_out);  edge_point / edge_kf / edge_feat [E] sorted by (point, keyframe) strictly ascending
 *   params.robust != 0: Huber edges with deltas (float) sqrt(huber2_mono / huber2_stereo), 6l's quadratic form entry for entry;
 *   robust == 0 (the loop path): base_binary_edge.hpp:75-90 with Omega = invSigma2 I, and activeChi2 sums chi2 itself
 * Outputs: pose [K,7] doubles and pose_f32 their cast -- a fixed keyframe's row is its widened, normalised input; point [L,3] and
 *   point_f32; included [L]: 0 for a point without an edge (vbNotIncludedMP: the reference removes the vertex, this entry keeps it with
 *   zero blocks and x = 0; the caller does not write it back); chi2 [E] as the last computeActiveErrors left it; trace [iterations,4] per
 *   LM iteration run: trials, the lambda it left, currentChi, 0; stats [8]: 0 LM iterations, 1 trials, 2 rejected trials, 3 failed solves,
 *   4 flags, 5 free keyframes, 6 tiles the factorisation processes, 7 tiles of the dense lower triangle.  Flags: rfe_local_ba's 1, 2, 4, 8
 *   and 16; a solve also fails on a non-finite entry of L or of the solution (6m).
 * BOTH forms are synchronous, like rfe_local_ba: the LM loop runs on the host, plain launches on the ctx stream and one small pinned
 * read per linearisation and per trial; `stop` (a HOST pointer, pbStopFlag, may be NULL) is read where g2o's terminate() is.  The first
 * kernels validate the keyframe and edge tables and the host reads the verdict before anything indexes by them.  Both return the number
 * of LM iterations run (>= 0).  pose_f32, point_f32, chi2, trace, octave, uright may be NULL.
 * Refused (RFE_ERR_INVALID): K outside 1..RFE_GBA_MAX_KF, L outside 0..RFE_GBA_MAX_POINTS, E outside 0..RFE_GBA_MAX_EDGES, Nf < 0;
 *   iterations outside 0..RFE_GBA_MAX_ITERATIONS, max_trials < 0; a non-finite huber2 or user_lambda_init; a NULL required pointer, `fixed`
 *   among them; an nlevels outside 1..RFE_MAX_LEVELS; a kf_feat_off that decreases or leaves 0..Nf; an edge index out of range; edges not
 *   strictly ascending in (point, keyframe); more than RFE_GBA_MAX_PAIRS Schur pair entries (sum over the points of n (n + 1) / 2, n the
 *   point's edges on free keyframes; the cap keeps the pair workspace at 512 MiB).  Nothing is written then.
 * Workspace, grow-only: 648 bytes an observation, 268 a point, 12 K^2 for the block keys, 16 a Schur pair, and (24 ceil(P / 4))^2 doubles for the
 *   matrix of P free keyframes: about 2.3 GB with every cap reached (1.36 GB of it for E = 2^21 observations).
 * Out of scope: FullInertialBA, the merge overloads, EdgeSE3ProjectXYZToBody, KannalaBrandt8, the spanning-tree propagation of
 *   RunGlobalBundleAdjustment, an ordering other than ascending keyframe index. */
#define RFE_GBA_MAX_KF 1024
#define RFE_GBA_MAX_POINTS (1 << 18)
#define RFE_GBA_MAX_EDGES (1 << 21)
#define RFE_GBA_MAX_ITERATIONS 64
#define RFE_GBA_MAX_PAIRS (1 << 25)
#define RFE_GBA_FLAG_ENDED_REJECTED 1
#define RFE_GBA_FLAG_SOLVE_FAILED 2
#define RFE_GBA_FLAG_NONFINITE 4
#define RFE_GBA_FLAG_STOPPED 8
#define RFE_GBA_FLAG_NO_ITERATION 16
typedef struct rfe_global_ba_params {
    int32_t iterations;          /* optimizer.optimize(nIterations): 10 behind a loop, 20 at the monocular initialisation; 0 runs none */
    int32_t max_trials;          /* 0 = g2o's 10 */
    double user_lambda_init;     /* <= 0: g2o's 1e-5 max |diagonal| */
    int32_t robust;              /* bRobust */
    int32_t reserved;
    double huber2_mono, huber2_stereo; /* 5.99, 7.815: the Huber deltas are (float) sqrt of them; read when robust != 0 */
    const volatile uint8_t* stop;/* HOST pointer or NULL: pbStopFlag */
} rfe_global_ba_params;
int rfe_global_ba_dev(rfe_ctx* ctx, rfe_global_ba_params params, const float* kf_pose_dev, const float* kf_cam_dev, const int32_t* kf_nlevels_dev,
                      const float* kf_inv_level_sigma2_dev, const int32_t* kf_feat_off_dev, const uint8_t* fixed_dev, const float* kpts_un_dev,
                      const int32_t* octave_dev, const float* uright_dev, const float* xw_dev, const int32_t* edge_point_dev,
                      const int32_t* edge_kf_dev, const int32_t* edge_feat_dev, int K, int L, int E, int Nf, double* pose_dev, float* pose_f32_dev,
                      double* point_dev, float* point_f32_dev, uint8_t* included_dev, double* chi2_dev, double* trace_dev, int32_t* stats_dev);
int rfe_global_ba(rfe_ctx* ctx, rfe_global_ba_params params, const float* kf_pose, const float* kf_cam, const int32_t* kf_nlevels,
                  const float* kf_inv_level_sigma2, const int32_t* kf_feat_off, const uint8_t* fixed, const float* kpts_un, const int32_t* octave,
                  const float* uright, const float* xw, const int32_t* edge_point, const int32_t* edge_kf, const int32_t* edge_feat, int K, int L,
                  int E, int Nf, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* included, double* chi2, double* trace,
                  int32_t* stats);

/* ---- TwoViewReconstruction on the device: the monocular initialisation's H and F RANSAC in one call ----
 * TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:49-1221) behind the matcher: B problems (two frames each) per call.
 * The front normalises both frames' keypoints (Normalize, over ALL n1 / n2 keypoints), lays the matches out and resolves every
 * iteration's 8-set from the raw draws; one wave per (iteration, model) runs the 8-point DLT (ComputeH21 / ComputeF21) and scores it
 * over every match (CheckHomography / CheckFundamental); one workgroup per problem takes the FIRST maximum of each model, RH = SH /
 * (SH + SF), recomputes the winner's inlier flags and decomposes the chosen model into its 8 (ReconstructH) or 4 (ReconstructF) motion
 * hypotheses; one thread per (hypothesis, match) runs CheckRT's Triangulate and gates; one workgroup per problem makes the
 * reference's decision.  fp32, one rounding per operation; the outputs equal tests/two_view_ref.py bit for bit (6o states the
 * arithmetic and its departures: fixed-schedule one-sided Jacobi for Eigen's JacobiSVD, fixed evaluation orders, acos in double).
 * params [B] is a HOST array in both forms:
 *   fx fy cx cy; sigma (0 = 1.0); rh_threshold (0 = the reference's 0.50); min_parallax (0 = 1.0); min_triangulated (0 = 50);
 *   its = mMaxIterations (0 = 200; at most H); n1, n2: the keypoint counts of frame 1 and 2 (within N1max, N2max)
 *   kpts1 [B,N1max,2], kpts2 [B,N2max,2]  mvKeysUn of both frames
 *   S [B], pairs [B,Kmax,2]  the matches (i in frame 1, j in frame 2), i strictly ascending: exactly what rfe_match_dev writes; S is
 *                  clamped to 0..Kmax
 *   draws [B,H,8]  the raw rand() results (0 .. 2^31 - 1) of every iteration, in the reference's order: a draw r picks position
 *                  (int)(((double)r / 2147483648.0) * size) (clamped to the list) of the swap-with-back list of :99-115.  Exactly 8 its
 *                  draws are consumed.
 * Outputs per problem: R21 [9] row-major, t21 [3] (the identity and 0 when the call answers false); p3d [N1max,3] and triangulated
 *   [N1max] indexed by the feature of frame 1 (rows 0..n1-1 are written: zero where nothing was triangulated and when the call answers
 *   false); inliers_h, inliers_f [Kmax] the best hypothesis' vbMatchesInliers per match (rows 0..S-1); scores [H,2] currentScore of every
 *   iteration < its, H then F; models [2,9] the chosen H21 and F21 (zero when no iteration won); cand [8,16] per motion hypothesis R
 *   [9], t [3], nGood, parallax, 0, 0 (the rows of the hypotheses that ran);
 *   stats [16]: 0 the return value, 1 model (0 none, 1 H, 2 F), 2 N, 3 / 4 the winning iteration of H / F (-1 none), 5 / 6 their inlier
 *   counts, 7 the chosen motion hypothesis (-1 none), 8 / 9 / 10 the bits of SH / SF / RH, 11 the exit (0 success, 1 SH + SF == 0, 2 the
 *   singular-value ratios of ReconstructH, 3 no clear winner, 4 too few points, 5 parallax), 12 flags (1 N < 8, 2 a pair index outside
 *   n1 / n2 -- either answers false without an iteration --, 4 a non-finite score), 13.. 0.
 * Every output except R21, t21 and stats may be NULL.  The _dev form is asynchronous on the ctx stream: no host synchronisation, no
 * host read of device data, no allocation once the workspace has the call's size; five launches.  The host form stages its arrays and
 * returns stats[0] of problem 0 (0 when B = 0).
 * Refused (RFE_ERR_INVALID): B outside 0..16; N1max, N2max or Kmax outside 0..4096; H outside 1..1024; its outside 0..H (200 > H when
 *   its = 0); n1 / n2 outside their capacities; min_triangulated < 0; a NULL required pointer; host form only: a non-finite intrinsic
 *   or sigma.  Keypoints are not checked: a NaN runs through (every score is NaN, no iteration wins, the call answers false).
 * Out of scope: KannalaBrandt8::ReconstructWithTwoViews (it undistorts, then runs the same class). */
typedef struct rfe_two_view_params {
    float fx, fy, cx, cy, sigma, rh_threshold, min_parallax;
    int32_t min_triangulated, its, n1, n2;
} rfe_two_view_params;
int rfe_two_view_dev(rfe_ctx* ctx, const rfe_two_view_params* params, const float* kpts1_dev, const float* kpts2_dev, const int32_t* S_dev,
                     const int32_t* pairs_dev, const int32_t* draws_dev, int B, int N1max, int N2max, int Kmax, int H, float* R21_dev,
                     float* t21_dev, float* p3d_dev, uint8_t* triangulated_dev, uint8_t* inliers_h_dev, uint8_t* inliers_f_dev,
                     float* scores_dev, float* models_dev, float* cand_dev, int32_t* stats_dev);
int rfe_two_view(rfe_ctx* ctx, const rfe_two_view_params* params, const float* kpts1, const float* kpts2, const int32_t* S,
                 const int32_t* pairs, const int32_t* draws, int B, int N1max, int N2max, int Kmax, int H, float* R21, float* t21, float* p3d,
                 uint8_t* triangulated, uint8_t* inliers_h, uint8_t* inliers_f, float* scores, float* models, float* cand, int32_t* stats);

/* ---- place recognition: ComputeBoW3 and the keyframe database's scores on the device ----
 * Frame::ComputeBoW3 / KeyFrame::ComputeBoW3 (src/Frame.cc:1044-1054) = binarize_descriptors + DBoW3::Vocabulary::transform
 * (Thirdparty/DBoW3/src/Vocabulary.cpp:752-874); KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates
 * (src/KeyFrameDatabase.cc:660-740, :1045-1100) up to and including the L1 scores.
 * The reference's own bodies behind this contract, as oracle/ref_classic/build_ref.py cuts or checks them (tests/test_ref_bow.py):
 *   Thirdparty/DBoW3/src/Vocabulary.cpp: the constructor :10-16, createScoringObject :48-80, the destructor :112-115, transform(features,
 *     v, fv, levelsup) :752-818, the per-feature overload with nid :836-874, toStream :1180-1257, fromStream :1335-1406;
 *   Thirdparty/DBoW3/src/DescManip.cpp: distance :92-130, toStream :249-258, fromStream :260-267;
 *   Thirdparty/DBoW3/src/BowVector.cpp: addWeight :34-46, addIfNotExist :50-58, normalize :62-84;
 *   Thirdparty/DBoW3/src/FeatureVector.cpp: addFeature :31-45;  Thirdparty/DBoW3/src/ScoringObject.cpp: L1Scoring::score :23-68;
 *   src/KeyFrameDatabase.cc: add :44-54, erase :65-85, the counting, gating and scoring of DetectNBestCandidates_sp :661-739 and of
 *     DetectRelocalizationCandidates :1047-1099.
 *
 * A vocabulary is a tree in flat host arrays (rfe_bow_vocab_desc): node 0 is the root, children [child_offsets[i], child_offsets[i + 1])
 * are node i's children in their stored order, desc [n_nodes, D] u8 the node descriptors (row 0 is ignored), weight [n_nodes] f64,
 * word_id [n_nodes] (-1 for inner nodes), parent [n_nodes] (the root's entry is ignored).  weighting / scoring carry DBoW3's enum values.
 * Leaves may lie at different depths.  Refused (RFE_ERR_INVALID, rfe_last_error): n_nodes outside 1..2^24; D not a multiple of 8 or
 * outside 8..256; scoring != RFE_BOW_L1_NORM; weighting outside 0..3; child_offsets not ascending from 0 to n_nodes - 1; a child index
 * out of range or the root; a node with two parents; parent[] disagreeing with children[]; a node the root does not reach; a childless
 * node without a word id.
 * rfe_bow_vocab_load reads DBoW3's UNCOMPRESSED binary stream (Vocabulary::toStream(.., false)): u64 88877711233, u8 compressed, u32
 * nnodes, i32 k, L, scoring, weighting, then per node but the root u32 id, u32 parent, f64 weight, i32 cols, rows, type and cols bytes,
 * then u32 nwords and (u32 word, u32 node) pairs; children in the order of the file.  RFE_ERR_IO: the file cannot be read, is not such
 * a stream, is compressed (re-save it uncompressed; there is no quicklz here), holds a descriptor that is not one CV_8U row of one common
 * width, or a count, id or length the file's size does not bear out.  Then rfe_bow_vocab_create's checks. */
#define RFE_BOW_TF_IDF 0
#define RFE_BOW_TF 1
#define RFE_BOW_IDF 2
#define RFE_BOW_BINARY 3
#define RFE_BOW_L1_NORM 0
typedef struct rfe_bow_vocab rfe_bow_vocab;
typedef struct rfe_bow_db rfe_bow_db;
typedef struct rfe_bow_vocab_desc {
    int32_t k, L, weighting, scoring;
    int32_t n_nodes, D;
    const int32_t* parent;
    const int32_t* child_offsets;
    const int32_t* children;
    const uint8_t* desc;
    const double* weight;
    const int32_t* word_id;
} rfe_bow_vocab_desc;
int rfe_bow_vocab_create(rfe_ctx* ctx, const rfe_bow_vocab_desc* desc, rfe_bow_vocab** out);
int rfe_bow_vocab_load(rfe_ctx* ctx, const char* path, rfe_bow_vocab** out);
void rfe_bow_vocab_destroy(rfe_bow_vocab* vocab);
/* info [8]: k, L, n_nodes, n_words (childless nodes), D, weighting, scoring, depth of the deepest leaf */
int rfe_bow_vocab_info(const rfe_bow_vocab* vocab, int32_t* info);
/* Vocabulary::transform(features, v, fv, levelsup) of N features: desc_f32 [N,256] floats, binarised as rfe_binarize_descriptors does
 * (byte = value > 0, NaN -> 0; the vocabulary's D must be 256), or desc_u8 [N,D] bytes as they are -- exactly one of the two non-NULL.
 * Per feature the descent: from the root, at every node the child with the smallest distance (popcount of the xor over the D bytes),
 * the first of equal ones, until a childless node: word [N] = its word id, weight [N] = its weight, node [N] = the node passed at depth
 * L - levelsup (the root when that is <= 0; the leaf's own node id when the leaf is shallower -- the reference leaves *nid unwritten
 * there).  Features with weight > 0 enter the results: bow_word ascending with bow_value = the weights of the word's features summed in
 * feature order (TF_IDF, TF) or the first one (IDF, BINARY), then every value divided by their sum taken in word order (when > 0), all
 * in IEEE double, one rounding per operation; fv_node ascending, node i's features fv_feat[fv_offsets[i] .. fv_offsets[i + 1]) ascending.
 * word / node / weight may be NULL; the others need room for N (fv_offsets N + 1) entries and are written up to bow_n / fv_n /
 * fv_offsets[fv_n] only.  N == 0 or every feature stopped: bow_n = fv_n = 0.  The _dev form is asynchronous on the ctx stream; the
 * host form returns bow_n.  Refused (RFE_ERR_INVALID): N outside 0..4096; both or neither descriptor pointer; desc_f32 with D != 256;
 * a vocabulary created on another device; desc_f32_dev not 16-byte or desc_u8_dev not 8-byte aligned. */
int rfe_bow_transform_dev(rfe_ctx* ctx, const rfe_bow_vocab* vocab, const float* desc_f32_dev, const uint8_t* desc_u8_dev, int N, int levelsup,
                          int32_t* word_dev, int32_t* node_dev, double* weight_dev, int32_t* bow_n_dev, int32_t* bow_word_dev,
                          double* bow_value_dev, int32_t* fv_n_dev, int32_t* fv_node_dev, int32_t* fv_offsets_dev, int32_t* fv_feat_dev);
int rfe_bow_transform(rfe_ctx* ctx, const rfe_bow_vocab* vocab, const float* desc_f32, const uint8_t* desc_u8, int N, int levelsup,
                      int32_t* word, int32_t* node, double* weight, int32_t* bow_n, int32_t* bow_word, double* bow_value, int32_t* fv_n,
                      int32_t* fv_node, int32_t* fv_offsets, int32_t* fv_feat);
/* The keyframe database: BoW vectors (ascending words, values) in a device store that grows geometrically; an entry id is the number
 * of adds before it since creation or the last clear, and stays valid through later adds and erases (an erased entry's words stay in the
 * store until rfe_bow_db_clear).  rfe_bow_db_size = entry ids issued, erased ones included: the length of the per-entry arrays below.
 * rfe_bow_db_query*: common [size] = the query's words present in the entry (0 for an erased one); over the entries that are not excluded
 * (exclude [size] u8, may be NULL): max_common, n_sharing = entries with common > 0; min_common = (int)(max_common * 0.8f); scored [size]
 * = not excluded and common > min_common; score [size] = L1Scoring::score(query, entry) where scored -- the terms |v - w| - |v| - |w|
 * of the common words summed in ascending word order, then -sum / 2, in IEEE double -- and not written elsewhere.  stats [4] = max_common,
 * min_common, n_sharing, n_scored.  The query's words must ascend (as rfe_bow_transform writes them); nq within 0..4096, an entry's n
 * within 0..4096.  The _dev forms are asynchronous on the stream of the ctx the database was created on, except that an add that grows
 * the store waits for that stream first.  The host query returns n_scored. */
int rfe_bow_db_create(rfe_ctx* ctx, rfe_bow_db** out);
void rfe_bow_db_destroy(rfe_bow_db* db);
int rfe_bow_db_add_dev(rfe_bow_db* db, const int32_t* word_dev, const double* value_dev, int n, int32_t* entry_id);
int rfe_bow_db_add(rfe_bow_db* db, const int32_t* word, const double* value, int n, int32_t* entry_id);
int rfe_bow_db_erase(rfe_bow_db* db, int32_t entry_id);
int rfe_bow_db_clear(rfe_bow_db* db);
int rfe_bow_db_size(const rfe_bow_db* db);
int rfe_bow_db_query_dev(rfe_bow_db* db, const int32_t* q_word_dev, const double* q_value_dev, int nq, const uint8_t* exclude_dev,
                         int32_t* common_dev, uint8_t* scored_dev, double* score_dev, int32_t* stats_dev);
int rfe_bow_db_query(rfe_bow_db* db, const int32_t* q_word, const double* q_value, int nq, const uint8_t* exclude, int32_t* common,
                     uint8_t* scored, double* score, int32_t* stats);

/* ---- multi-device pool (BASELINE configs[3] for a C / C++ host) ----
 * The reference runs on ONE device (device_id = 0, src/Extractors/superpoint_onnx.cc:19, src/Matchers/lightglue_onnx.cpp:24) and
 * is a C++ program (src/Tracking.cc:645-651); a pool gives such a host the frame sharding of rover-slam_amd/sharding.py without
 * Python: one ctx + one host worker thread per member device.  A stream of F frames has F - 1 consecutive pairs; they are split
 * as evenly as possible (rfe_pool_shard), member r extracts its pairs' frames -- ONE overlap frame with its neighbour, no
 * inter-device dependency -- and matches them; every member's results are then gathered into one root buffer on member 0's device
 * in global frame / pair order and copied to the caller's HOST arrays (layouts as rfe_extract_match_stream_dev with B = F;
 * score / desc may be NULL = not gathered).
 * transport: RFE_POOL_RCCL = grouped ncclSend / ncclRecv into the root (librccl is dlopen'ed at pool creation; needs pairwise
 * distinct devices), RFE_POOL_COPY = peer / device-to-device copies issued by the root (members may share a device),
 * RFE_POOL_AUTO = RCCL when the pool has more than one member and the communicators are up, else COPY.
 * `devices` may name one device several times (functional tests on a one-GPU box; weights are then shared, see rfe_weights_id).
 * A pool is single-caller like a ctx.  rfe_pool_ctx exposes a member's ctx (options, profiling); do not run it while a pool call
 * is in flight. */
typedef struct rfe_pool rfe_pool;
#define RFE_POOL_AUTO 0
#define RFE_POOL_RCCL 1
#define RFE_POOL_COPY 2
int rfe_pool_create(const int* devices, int n, rfe_pool** out);
void rfe_pool_destroy(rfe_pool* pool);
const char* rfe_pool_last_error(rfe_pool* pool); /* pool may be NULL: last error of a failed rfe_pool_create */
int rfe_pool_size(rfe_pool* pool);
rfe_ctx* rfe_pool_ctx(rfe_pool* pool, int member);
int rfe_pool_has_rccl(rfe_pool* pool);           /* 1 = RCCL communicators are up */
int rfe_pool_set_weights(rfe_pool* pool, int kind, const float* blob, int64_t count);
int rfe_pool_load_weights(rfe_pool* pool, const char* sp_path, const char* lg_path);
int rfe_pool_set_option(rfe_pool* pool, int option, int value);
int rfe_pool_set_hparams(rfe_pool* pool, const rfe_hparams* in);   /* every member; rfe_pool_load_weights applies a v2 file's values by itself */
/* the sharding rule itself (pure function, no device): member `member` of n extracts frames [first_frame, first_frame + frames)
 * of an F-frame stream and owns `pairs` consecutive pairs starting at first_frame (frames = pairs + 1; 0 / 0 = idle member) */
int rfe_pool_shard(int F, int n, int member, int* first_frame, int* frames, int* pairs);
int rfe_pool_extract_match_stream(rfe_pool* pool, const uint8_t* img_host, int H, int W, int stride, int F, int Kmax, float thr,
                                  float filter_thr, int transport, int32_t* n, int32_t* kxy, float* score, float* desc,
                                  int32_t* S, int32_t* pairs, float* ms);

/* ---- per-stage timing (hipEvent on the ctx stream), for bench.py's roofline object ----
 * Enable, run, then read back: names is a ';'-separated list of stage names, ms / calls the
 * accumulated time and launch count per stage since the last reset.
 * rfe_profile_filter restricts the events to one stage (NULL or "" = all stages): each pair of events keeps
 * consecutive kernels from overlapping their launch and drain (about 2 % of a batched step when every stage is
 * instrumented), so a throughput measurement instruments only the kernel it reports. */
int rfe_profile_enable(rfe_ctx* ctx, int on);
int rfe_profile_filter(rfe_ctx* ctx, const char* stage);
int rfe_profile_reset(rfe_ctx* ctx);
int rfe_profile_read(rfe_ctx* ctx, char* names, size_t names_cap, double* ms, int64_t* calls, int cap);

/* ---- kernel-level test hooks (device pointers, synchronous): used only by tests/ ----
 * NHWC activations, canonical weight layouts as in the oracle. */
int rfe_k_conv3x3(rfe_ctx* ctx, const float* in_dev, int B, int H, int W, int Cin,
                  const float* w_oihw_host, const float* bias_host, int Cout, int relu, int pool,
                  float* out_dev);
int rfe_k_linear(rfe_ctx* ctx, const float* a_dev, int M, int K, const float* w_nk_host,
                 const float* bias_host, int N, int relu, float* out_dev);
int rfe_k_scoremap(rfe_ctx* ctx, const uint8_t* img_dev, int H, int W, int stride, int B,
                   float* scoremap_dev /*[B,Hs,Ws] pre-NMS, Hs = 8*(H/8), Ws = 8*(W/8)*/,
                   float* nms_dev /*[B,Hs,Ws] post-NMS+border*/, float* descmap_dev /*[B,H/8,W/8,256]*/);
/* The sparse descriptor head of calls with more than four frames (descriptor stages only on the cells that keypoints sample), alone and through the
 * forward's own code, behind the backbone of B frames and for caller-provided keypoints n_dev [B], kxy_dev [B,Kmax,2].  poison != 0: its workspace is
 * filled with NaN words first.  Outputs (each may be NULL): cell_row_dev [B,(H/8)*(W/8)] row of a cell within its frame or -1, count_dev [B] live rows
 * per frame, rows_dev [B*cap,256] with cap = min(4*Kmax, (H/8)*(W/8)): the normalised descriptor rows, frame after frame without gaps, ascending cell order
 * inside a frame (sum(count) rows are written), desc_dev [B,Kmax,256] sampled through cell_row. */
int rfe_k_sparse_desc(rfe_ctx* ctx, const uint8_t* img_dev, int H, int W, int stride, int B, int Kmax, const int32_t* n_dev, const int32_t* kxy_dev,
                      int poison, int32_t* cell_row_dev, int32_t* count_dev, float* rows_dev, float* desc_dev);
/* keypoint selection alone on a post-NMS map (H, W multiples of 8 as the score-map frame always is): n [B], kxy [B,Kmax,2], score [B,Kmax] */
int rfe_k_select(rfe_ctx* ctx, const float* nms_dev /*[B,H,W]*/, int B, int H, int W, int Kmax, float thr, int topk_always,
                 int32_t* n_dev, int32_t* kxy_dev, float* score_dev);
/* the same through the form one to four frames take in the forward: an UNORDERED list of 64-bit candidate keys (as the fused detector tail leaves it), ranked */
int rfe_k_select_keys(rfe_ctx* ctx, const float* nms_dev /*[B,H,W], B <= 4*/, int B, int H, int W, int Kmax, float thr, int topk_always,
                      int32_t* n_dev, int32_t* kxy_dev, float* score_dev);
int rfe_k_lightglue_taps(rfe_ctx* ctx, const float* k0n, const float* k1n, const float* d0,
                         const float* d1, int M, int N, float* x0_dev, float* x1_dev,
                         float* scores_dev /*[M,N]*/);

/* One FFN block of LightGlue with the loaded weights: out = x + ffn.3(gelu(LayerNorm(ffn.0([x | second])))) for `rows` token rows
 * (x, second, out: device [rows,256]; out may not alias x), self (cross = 0) or cross block of `layer`.  Goes through the forward's
 * own code, so the row count selects the tiling: >= 32768 rows = throughput tiles with the fused LayerNorm + GELU. */
int rfe_k_lightglue_ffn(rfe_ctx* ctx, int layer, int cross, const float* x_dev, const float* second_dev, int rows, float* out_dev);
/* The fused attention alone: out[seq][q][head*64 + d] = softmax(Q K^T / 8) V per (sequence, head), 4 heads of 64 (device pointers, row
 * stride ld floats for q / k / v, out [nseq*Lq, 256]); qlen / klen: valid rows per sequence or NULL, kv_map: sequence -> sequence whose
 * k / v it attends to or NULL, rope: LightGlue's rotary table [nseq*Lq, 32] of (cos, sin) pairs applied to q and k, or NULL.  Goes through
 * the forward's launcher, so nseq * Lq and RFE_OPT_LG_FP16X2 select the kernel exactly as inside a match call. */
int rfe_k_attention(rfe_ctx* ctx, const float* q_dev, const float* k_dev, const float* v_dev, int ld, float* out_dev, int nseq, int Lq, int Lk,
                    const int32_t* qlen_dev, const int32_t* klen_dev, const int32_t* kv_map_dev, const float* rope_dev);
/* Both directions of one LightGlue cross block, through the forward's own code: qk_v_dev [2*P*L, ld] rows [qk (256) | v (256) | ...] in the side-major
 * layout (sequence p < P is side 0 of pair p and attends to sequence p + P, and back), lens_dev [2*P] valid rows, out_dev [2*P*L, 256]; ld >= 512,
 * ld % 4 == 0, L % 4 == 0, 4 <= L <= 4096.  form 0: the form a match call would choose at (P, L); 1: the shared-logit form (side 0 writes each pair's
 * logits out, side 1 reads them back) at any shape; 2: the generic form (every direction forms its own logits).  The LightGlue workspace, logit scratch included, is filled
 * with NaN before the launches.  A ctx is enough, no weights. */
int rfe_k_cross_attention(rfe_ctx* ctx, const float* qk_v_dev, int ld, float* out_dev, int P, int L, const int32_t* lens_dev, int form);
/* Projection + attention of one self block with the loaded weights, through the forward's own code: x_dev [nseq*L, 256] token rows, csn_dev [nseq*L, 32]
 * (cos, sin) rotary pairs, lens_dev [nseq] valid rows; qkv_out_dev [nseq*L, 768] = [q | k | v] as the attention reads them, ctx_out_dev [nseq*L, 256]
 * (either may be NULL).  nseq * L selects the path as inside a match call: throughput shapes rotate q | k in the projection's epilogue (gemm.hip) and run
 * the LDS-DMA attention kernel, one / few pairs take gemm_lat.hip + lg_attention_lat.hip; *qk_rotated = 1 when qkv_out's q | k are rotated (0: the
 * fallback that rotates on load).  L % 4 == 0. */
int rfe_k_lightglue_self_attention(rfe_ctx* ctx, int layer, const float* x_dev, const float* csn_dev, const int32_t* lens_dev, int nseq, int L,
                                   float* qkv_out_dev, float* ctx_out_dev, int32_t* qk_rotated);
/* LightGlue's assignment stage alone, through the forward's own code, on caller-provided inputs (device pointers; a ctx is enough, no weights):
 * sim_dev [P,L,L] similarities, x_dev [2,P,L,256] final token states (side-major: all side-0 sequences, then all side-1), wm_dev [256] / bm_dev [1] the
 * matchability head, lens_dev [2P] valid rows (all m, then all n; each within [0, L]); L % 4 == 0, 4 <= L <= 4096; thr the match filter, cap the list
 * capacity per pair.  (P, L) selects the kernels as inside a match call.  Before the stage runs, every output buffer is filled with the 32-bit word
 * `sentinel`, so words the stage did not write read back as the sentinel.  Outputs (each may be NULL): z_dev [2,P,L] log sigmoid of the matchability
 * logits (written for EVERY padded row), rowlse_dev / collse_dev / mx0_dev [P,L] f32, a0_dev / a1_dev [P,L] i32, S_dev [P], pairs_dev [P,cap,2],
 * ms_dev [P,cap], and the log-assignment dump scores_dev: [P,L,L] (scores_pair < 0) or [L,L] of pair `scores_pair`; only live m x n blocks are written. */
int rfe_k_lightglue_assign(rfe_ctx* ctx, const float* sim_dev, const float* x_dev, const float* wm_dev, const float* bm_dev, const int32_t* lens_dev,
                           int P, int L, float thr, int cap, int scores_pair, int32_t sentinel, float* z_dev, float* rowlse_dev, float* collse_dev,
                           float* mx0_dev, int32_t* a0_dev, int32_t* a1_dev, int32_t* S_dev, int32_t* pairs_dev, float* ms_dev, float* scores_dev);
/* The gates of rfe_two_view without an SVD in front of them, through the device functions the kernels use.  HOST pointers,
 * synchronous, n <= 4096; pts [n,4] = u1 v1 u2 v2 of every match.
 * rfe_k_two_view_check: CheckHomography (model 0; H12 is the cofactor inverse of M) or CheckFundamental (model 1) of ONE model M [9]:
 *   contrib [n] what each match adds to the score, inl [n] its flag.
 * rfe_k_two_view_check_rt: CheckRT of ONE motion hypothesis Rt [12] = R row-major | t with K4 = fx fy cx cy and th2: code [n] (0 not
 *   counted, 1 counted in nGood without vbGood, 2 counted and vbGood), cosp [n] cosParallax, p3d [n,3]. */
int rfe_k_two_view_check(rfe_ctx* ctx, int model, const float* M, float sigma, const float* pts, int n, float* contrib, uint8_t* inl);
int rfe_k_two_view_check_rt(rfe_ctx* ctx, const float* Rt, const float* K4, float th2, const float* pts, int n, uint8_t* code, float* cosp,
                            float* p3d);
/* The float chi2 classification of rfe_pose_inertial_optimization behind round `round` (0..3) or its recovery pass (round 4),
 * through the device functions the kernel uses, of n edges at ONE camera pose view [12] = Rcw row-major | tcw (doubles).  HOST pointers,
 * synchronous, 1 <= n <= 4096; every row is an edge.  outlier_in [n]: the flags before (a flagged edge recomputes its error at the view, any
 * other is compared at chi2_in [n]).  code [n]: rounds 0..3 the new flag; round 4 bit 0 the flag afterwards, bit 1 the edge counts in nBad.
 * chi2_out [n]: the float that was compared. */
int rfe_k_pose_inertial_classify(rfe_ctx* ctx, const rfe_pose_inertial_params* params, int mode, int round, const double* view, const float* kpts_un,
                                 const int32_t* octave, const float* uright, const float* xw, const float* track_depth, const uint8_t* outlier_in,
                                 const float* chi2_in, int n, uint8_t* code, float* chi2_out);
/* One-shot tap for the NEXT LightGlue forward of this ctx, whichever entry point runs it (rfe_match[_dev] with P pairs,
 * rfe_extract_match_stream_dev, rfe_stereo_frame_dev) and therefore whichever tiling it selects: after the last layer the final
 * token states of pair `pair` are copied to x0_dev / x1_dev ([L,256] each, L = max(Mmax,Nmax) rounded up to 4; rows past the
 * pair's keypoint counts are padding) and its log-assignment matrix to scores_dev ([L,L], row stride L; only the m x n block is
 * written).  Any pointer may be NULL; pair < 0 disarms.  A pair index >= P of the next forward is ignored. */
int rfe_k_set_lightglue_tap(rfe_ctx* ctx, int pair, float* x0_dev, float* x1_dev, float* scores_dev);
/* One-shot hook for the NEXT rfe_global_ba / rfe_global_ba_dev of this ctx: when that call is given a `stop` pointer, the library
 * itself writes 1 through it behind the call's `trials`-th trial (counted over the whole call), in front of the read of `stop` that
 * follows a trial -- "pbStopFlag set while the optimisation runs", at a known trial.  trials <= 0 disarms.  The hook is taken by the
 * first call that passes its argument checks, whatever becomes of that call. */
int rfe_k_global_ba_stop_after(rfe_ctx* ctx, int trials);
/* Fault injection for the pool's RCCL gather: the NEXT gather of `member` fails inside its ncclGroup (as a refused ncclSend would).  The
 * failing member aborts every member's communicator, nobody is left waiting in a collective, and the call delivers its results through
 * the COPY transport (RFE_POOL_AUTO) or reports the failure (RFE_POOL_RCCL); later calls use COPY.  tests/test_pool.py. */
int rfe_k_pool_inject_gather_failure(rfe_pool* pool, int member);
/* The ONNX reader without a ctx (and without a GPU): `path` of `kind` -> blob [rfe_weight_count(kind)] and that kind's fields of *hp (weights_only != 0:
 * the initializers alone, no hyper-parameter readers).  RFE_OK, or RFE_ERR_IO with the reason in err.  tests/test_onnx_cpp.py holds it bit for bit
 * against rover-slam_amd/onnx_weights.py. */
int rfe_k_onnx_convert(const char* path, int kind, int weights_only, float* blob, rfe_hparams* hp, char* err, int errlen);
/* The vocabulary reader and rfe_bow_vocab_create's checks without a ctx (and without a GPU): hdr [6] = k, L, weighting, scoring, n_nodes, D
 * of the stream at `path`; with the array pointers non-NULL (sized from a first call with all of them NULL) the tree as rfe_bow_vocab_desc
 * lays it out.  RFE_OK, or RFE_ERR_IO / RFE_ERR_INVALID with the reason in err. */
int rfe_k_bow_vocab_read(const char* path, int32_t* hdr, int32_t* parent, int32_t* child_offsets, int32_t* children, uint8_t* desc,
                         double* weight, int32_t* word_id, char* err, int errlen);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_FE_H */
