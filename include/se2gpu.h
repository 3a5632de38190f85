/* se2gpu.h - C ABI of the MI355X-native se2lam hot path (libse2gpu.so).
 *
 * The reference (izhengfan/se2lam) has no plugin / FFI layer: the boundary of its hot path
 * is three C++ header surfaces.  This C ABI is what a binding for those
 * surfaces calls; include/se2lam_amd/{ORBextractor,ORBmatcher,optimizer}.h are header-only C++
 * adapters over it that keep the reference's names and argument meaning.
 *
 * Conventions: every function returns an int status (SE2GPU_OK = 0, negative = error) and never
 * throws; the caller owns all host buffers; a handle owns its device memory and HIP stream and is
 * NOT thread-safe (one handle per calling thread, as the reference uses one ORBextractor per
 * thread and one SlamOptimizer per localBA call).  There is no CPU fallback: without a visible
 * gfx950 device every compute entry point returns SE2GPU_ERR_NO_DEVICE.
 */
#ifndef SE2GPU_H
#define SE2GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE2GPU_OK 0
#define SE2GPU_ERR_INVALID (-1)    /* bad argument / handle / id                      */
#define SE2GPU_ERR_NO_DEVICE (-2)  /* no HIP device (the library has no CPU fallback)  */
#define SE2GPU_ERR_HIP (-3)        /* a HIP runtime call failed; see se2gpu_last_error */
#define SE2GPU_ERR_CAPACITY (-4)   /* an internal or caller-supplied capacity overflowed */
#define SE2GPU_ERR_STATE (-5)      /* call sequence error (e.g. optimize before initialize) */

const char* se2gpu_last_error(void);    /* thread-local message of the last failing call */
int se2gpu_device_count(void);          /* number of visible HIP devices (0 = none)      */
const char* se2gpu_version(void);

/* ------------------------------------------------------------------------------------------
 * ORB extractor  -  replaces se2lam::ORBextractor
 *   ctor          /root/reference/include/se2lam/ORBextractor.h:44, src/ORBextractor.cpp:463-520
 *   operator()    /root/reference/include/se2lam/ORBextractor.h:49-51, src/ORBextractor.cpp:727-788
 * ------------------------------------------------------------------------------------------ */
typedef struct se2gpu_orb se2gpu_orb;

typedef struct se2gpu_orb_params {   /* defaults of ORBextractor.h:44 */
    int32_t nfeatures;     /* 1000 */
    float scale_factor;    /* 1.2f */
    int32_t nlevels;       /* 8    */
    int32_t score_type;    /* cv::ORB enum: 1 = FAST_SCORE (the reference's default), 0 = HARRIS_SCORE */
    int32_t fast_th;       /* 20   */
    int32_t max_rows, max_cols;  /* largest image the handle will see (0,0 -> 480,640) */
    int32_t max_batch;     /* frames per batched call (0 -> 1) */
} se2gpu_orb_params;

/* Layout-compatible with cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct se2gpu_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} se2gpu_keypoint;

int se2gpu_orb_create(const se2gpu_orb_params* params, se2gpu_orb** out);
void se2gpu_orb_destroy(se2gpu_orb* h);
int se2gpu_orb_levels(const se2gpu_orb* h);            /* GetLevels()      ORBextractor.h:53 */
float se2gpu_orb_scale_factor(const se2gpu_orb* h);    /* GetScaleFactor() ORBextractor.h:56 */

/* operator()(image, mask, keypoints, descriptors): `img` is a rows x cols CV_8UC1 host image with
 * row pitch `step`; `mask` is accepted and ignored, as in the reference (its cellMask never reaches cv::FAST,
 * ORBextractor.cpp:610-622; its only caller passes an empty mask, Frame.cpp:25).
 * Writes up to `cap` keypoints / cap*32 descriptor bytes, *n_out = number of keypoints.
 * An empty image (rows==0 || cols==0) returns OK with *n_out = 0 (ORBextractor.cpp:730-731). */
int se2gpu_orb_extract(se2gpu_orb* h, const uint8_t* img, int rows, int cols, size_t step, const uint8_t* mask,
                       se2gpu_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* Batched, device-resident form used for throughput (frames are independent):
 * d_imgs  = nframes contiguous rows x cols u8 images already in HBM (pitch = cols);
 * d_kps   = nframes * cap keypoints, d_desc = nframes * cap * 32 bytes, d_counts = nframes ints (device).
 * Asynchronous on the handle's stream; se2gpu_orb_sync() waits for it. */
int se2gpu_orb_extract_batch_device(se2gpu_orb* h, const uint8_t* d_imgs, int nframes, int rows, int cols,
                                    se2gpu_keypoint* d_kps, uint8_t* d_desc, int32_t* d_counts, int cap);
int se2gpu_orb_sync(se2gpu_orb* h);
int se2gpu_orb_set_stream(se2gpu_orb* h, void* hip_stream);  /* NULL -> the handle's own stream */

/* Introspection for the parity tests: copies pyramid level `level` of frame `frame` of the last call
 * (un-blurred if bit 0 of `blurred` is clear) into `out` (rows*cols of that level, tight pitch); rows and cols are set.
 * Bit 1 of `blurred` includes the 16 px reflect-101 frame: (rows + 32) x (cols + 32). */
int se2gpu_orb_debug_level(se2gpu_orb* h, int frame, int level, int blurred, uint8_t* out, size_t out_cap,
                           int* rows, int* cols);
/* FAST score map S of a level of the last call, same geometry as the level. */
int se2gpu_orb_debug_score(se2gpu_orb* h, int frame, int level, uint8_t* out, size_t out_cap, int* rows, int* cols);
/* The device routine behind both retainBest cuts (/root/reference/src/ORBextractor.cpp:692-694, 708-709 = cv::KeyPointsFilter::
 * retainBest + resize = std::nth_element by response, first n kept), run on caller data for the parity tests: `entries` (host,
 * in / out) are n values whose HIGH 32 bits are the comparison key (larger = better response) and whose low 32 bits travel
 * along; on return they are permuted exactly as libstdc++'s std::nth_element(first, first + nth, last, key greater) leaves
 * them.  force_global != 0 runs the in-place global-memory path that cells beyond the LDS capacity take. */
int se2gpu_orb_debug_nth_element(uint64_t* entries, int n, int nth, int force_global);

/* Camera model of the first step of Frame::Frame (the reference's src/Frame.cpp:19-25): cv::undistort(im, img, Kcam, Dcam)
 * in front of the extractor.  d holds OpenCV's order k1, k2, p1, p2 [, k3 [, k4, k5, k6]]; nd is 4, 5 or 8 (the thin-prism
 * and tilt models, 12 / 14 coefficients, are refused), entries from nd on are ignored.  The arithmetic is OpenCV 3.2's,
 * restated in DESIGN.md ("Camera undistortion"). */
typedef struct se2gpu_camera {
    float fx, fy, cx, cy;
    float d[8];
    int32_t nd;
} se2gpu_camera;

/* The fixed-point maps cv::undistort builds for a rows x cols image (initUndistortRectifyMap, CV_16SC2 + CV_16UC1, in stripes):
 * map_xy = rows * cols * 2 int16 (source column, source row), map_frac = rows * cols uint16 ((fy5 << 5) | fx5).  Host code, no device. */
int se2gpu_undistort_map(const se2gpu_camera* cam, int rows, int cols, int16_t* map_xy, uint16_t* map_frac);
/* cv::undistortPoints(src, dst, K, D, Mat(), K) for n points (x, y floats; xy_out may be xy_in).  Host code, no device. */
int se2gpu_undistort_points(const se2gpu_camera* cam, const float* xy_in, int n, float* xy_out);
/* A handle with a camera treats the images of se2gpu_orb_extract / se2gpu_orb_extract_batch_device as RAW camera images:
 * a remap kernel (INTER_LINEAR, BORDER_CONSTANT 0) undistorts them on the device in front of the pyramid, and level 0 of
 * se2gpu_orb_debug_level is the undistorted image.  The maps of an image size are built at the first extract of that size
 * and kept.  NULL takes the camera away again (the default: images are used as they come).  Waits for the handle's work. */
int se2gpu_orb_set_camera(se2gpu_orb* h, const se2gpu_camera* cam);

/* ------------------------------------------------------------------------------------------
 * ORB matcher  -  replaces se2lam::ORBmatcher
 *   DescriptorDistance   /root/reference/src/ORBmatcher.cpp:110-126
 *   MatchByWindow        /root/reference/src/ORBmatcher.cpp:278-381   (+ Frame::GetFeaturesInArea,
 *                        PosInGrid: /root/reference/src/Frame.cpp:209-286)
 *   MatchByProjection    /root/reference/src/ORBmatcher.cpp:383-454
 *   SearchByBoW          /root/reference/src/ORBmatcher.cpp:128-276
 * ------------------------------------------------------------------------------------------ */
int se2gpu_hamming(const uint8_t* a, const uint8_t* b);  /* host utility, 256-bit Hamming distance */
/* ORBmatcher::ComputeThreeMaxima (/root/reference/include/se2lam/ORBmatcher.h:57, src/ORBmatcher.cpp:64-105): host utility
 * over the bin COUNTS (histo[i].size()); ind1..3 in/out, the reference's callers start them at -1 */
int se2gpu_three_maxima(const int32_t* counts, int L, int* ind1, int* ind2, int* ind3);

typedef struct se2gpu_matcher se2gpu_matcher;
int se2gpu_matcher_create(int max_features, int max_batch, se2gpu_matcher** out);
void se2gpu_matcher_destroy(se2gpu_matcher* h);
int se2gpu_matcher_set_stream(se2gpu_matcher* h, void* hip_stream);
int se2gpu_matcher_sync(se2gpu_matcher* h);
/* Number of calls of this handle in which some query's search window held more than the 128 candidates the fast path lists
 * and was resolved by the exact grid scan instead (same result, a latency cliff on clustered features): lets the tracking
 * thread see the slow path, which is otherwise silent. */
int se2gpu_matcher_spill_calls(const se2gpu_matcher* h, long long* calls);

/* Image bounds / grid of Frame (Frame.cpp:37-44): minX,minY,maxX,maxY of the undistorted image. */
typedef struct se2gpu_frame_bounds {
    float min_x, min_y, max_x, max_y;
} se2gpu_frame_bounds;
/* Frame::computeBoundUn (Frame.cpp:183-200): the image rectangle when d[0] == 0 (the reference's rule, whatever the other
 * coefficients are), else the bounds of its four undistorted corners.  Host code, no device. */
int se2gpu_frame_bounds_un(const se2gpu_camera* cam, int rows, int cols, se2gpu_frame_bounds* out);

/* MatchByWindow(frame1, frame2, vbPrevMatched, winSize, vnMatches12, levelOffset, minLevel, maxLevel)
 * with ORBmatcher(nnratio, checkOri=true).  Host buffers.  prev_xy (n1 x 2 floats) is updated in place
 * as the reference updates vbPrevMatched (ORBmatcher.cpp:375-377).  matches12: n1 ints (-1 = none).
 * Returns the match count in *n_matches. */
int se2gpu_match_window(se2gpu_matcher* h, const se2gpu_frame_bounds* bounds,
                        const se2gpu_keypoint* kps1, const uint8_t* desc1, int n1,
                        const se2gpu_keypoint* kps2, const uint8_t* desc2, int n2,
                        float* prev_xy, int win_size, int level_offset, int min_level, int max_level,
                        float nnratio, int32_t* matches12, int* n_matches);

/* Batched device-resident MatchByWindow over `npairs` independent frame pairs.  Pair p matches
 * frame a[p] against frame b[p] of the same device arrays the batched extractor wrote
 * (d_kps: nframes*cap, d_desc: nframes*cap*32, d_counts: nframes).  prev_xy = keypoint positions of
 * frame a (Track::resetLocalTrack, Track.cpp:194).  d_matches12: npairs*cap ints, d_nmatches: npairs. */
int se2gpu_match_window_batch_device(se2gpu_matcher* h, const se2gpu_frame_bounds* bounds,
                                     const se2gpu_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                     int cap, const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs,
                                     int win_size, int level_offset, int min_level, int max_level, float nnratio,
                                     int32_t* d_matches12, int32_t* d_nmatches);

/* MatchByProjection(pNewKF, localMPs, winSize, levelOffset, vMatchesIdxMP) with ORBmatcher(nnratio).
 *  map points: mp_pos (m x 3 float, world), mp_desc (m x 32), mp_octave (m), mp_skip (m; 1 = the
 *  reference would `continue` at ORBmatcher.cpp:392-395: null / bad parallax / already observed);
 *  key frame:  Tcw (3x4 row-major float), K = fx, fy, cx, cy (float), kps/desc (n),
 *  kf_observed (n; 1 = hasObservation(idx), ORBmatcher.cpp:417).
 *  match_idx_mp: n ints (index into the map-point array, -1 = none). */
int se2gpu_match_projection(se2gpu_matcher* h, const se2gpu_frame_bounds* bounds,
                            const float* mp_pos, const uint8_t* mp_desc, const int32_t* mp_octave,
                            const uint8_t* mp_skip, int m,
                            const float* Tcw, float fx, float fy, float cx, float cy,
                            const se2gpu_keypoint* kps, const uint8_t* desc, const uint8_t* kf_observed, int n,
                            int win_size, int level_offset, float nnratio, int32_t* match_idx_mp, int* n_matches);

/* se2gpu_match_projection with every array in device memory, where se2gpu_mappoint_main_batch_device (d_mp_desc,
 * d_mp_octave) and the extractor (d_kps, d_desc of one frame) left them; Tcw (12 host floats) and the intrinsics travel by
 * value.  d_match_idx_mp: n ints, d_n_matches: one int, both device memory.  The same three launches as the host-buffer
 * call, asynchronous on the matcher's stream: no staging copy, no read-back and no wait; se2gpu_matcher_sync waits for it.
 * n == 0 only clears *d_n_matches.  The spill flag of the call (a query with more than 128 candidates) stays in the handle
 * until the next se2gpu_matcher_sync, which adds it to se2gpu_matcher_spill_calls; calls between two syncs count once.
 * SE2GPU_ERR_INVALID: a NULL handle, bounds, Tcw, d_n_matches or needed array; SE2GPU_ERR_CAPACITY: n > max_features. */
int se2gpu_match_projection_device(se2gpu_matcher* h, const se2gpu_frame_bounds* bounds,
                                   const float* d_mp_pos, const uint8_t* d_mp_desc, const int32_t* d_mp_octave,
                                   const uint8_t* d_mp_skip, int m,
                                   const float* Tcw, float fx, float fy, float cx, float cy,
                                   const se2gpu_keypoint* d_kps, const uint8_t* d_desc, const uint8_t* d_kf_observed, int n,
                                   int win_size, int level_offset, float nnratio,
                                   int32_t* d_match_idx_mp, int32_t* d_n_matches);

/* SearchByBoW(pKF1, pKF2, mapMatches12, bIfMPOnly) with ORBmatcher(nnratio, checkOri) - ORBmatcher.cpp:128-276.
 * The DBoW2::FeatureVector of each key frame (std::map<NodeId, std::vector<unsigned>>, computed by the host
 * vocabulary) is passed as CSR: fv_nodes[nn] ascending node ids, fv_ptr[nn+1], fv_idx[fv_ptr[nn]] feature indices.
 * has_mp1/2 (n1 / n2 bytes): 1 = the feature has a non-null map point (only read when mp_only != 0).
 * matches12: n1 ints, index into key frame 2 or -1 (the reference's std::map<int,int> as a dense array). */
int se2gpu_search_by_bow(se2gpu_matcher* h,
                         const se2gpu_keypoint* kps1, const uint8_t* desc1, int n1,
                         const int32_t* fv1_nodes, const int32_t* fv1_ptr, const int32_t* fv1_idx, int nn1,
                         const uint8_t* has_mp1,
                         const se2gpu_keypoint* kps2, const uint8_t* desc2, int n2,
                         const int32_t* fv2_nodes, const int32_t* fv2_ptr, const int32_t* fv2_idx, int nn2,
                         const uint8_t* has_mp2,
                         int mp_only, float nnratio, int check_orientation, int32_t* matches12, int* n_matches);

/* Batched device-resident SearchByBoW over `npairs` independent key-frame pairs: pair p is SearchByBoW(frame a[p],
 * frame b[p], .., mp_only) with ORBmatcher(nnratio, check_orientation).  Every pointer is device memory.  The frame arrays
 * are the ones se2gpu_orb_extract_batch_device writes (d_kps from f * cap, d_desc from f * cap * 32, d_counts[f]); the
 * feature vectors are the CSR se2gpu_bow_transform_batch_device writes (d_fv_nodes from f * cap, ascending; d_fv_ptr from
 * f * (cap + 1); d_fv_idx from f * cap; d_fv_nn[f]).  d_has_mp: nframes * cap bytes, 1 = the feature has a non-null map
 * point; read only when mp_only != 0 and may be NULL otherwise.  Row p of d_matches12 holds cap ints: entry i < counts[a[p]]
 * is the index into frame b[p] or -1, every entry from counts[a[p]] on is -1; d_nmatches[p] is the reference's return value.
 * The kernels never index outside the arrays, whatever the arrays hold: counts and nn are clamped to 0..cap, ptr values to
 * 0..cap, a segment whose end lies before its start is empty, a feature index outside the frame is skipped, and a pair that
 * names a frame outside 0..nframes-1 gives an all -1 row and count 0.
 * Asynchronous on the matcher's stream, as se2gpu_match_window_batch_device is: no read-back and no synchronise inside the
 * call; se2gpu_matcher_sync waits for it.  Ordering against the transform that writes the feature vectors is the caller's
 * job: se2gpu_matcher_set_stream(h, se2gpu_bow_stream(ctx)) puts both on one stream, or sync the context first.
 * The scratch (node pairs, their number, rotation bins and the 30 histogram counters of every pair) lives in the handle,
 * grows from npairs and cap alone and is reused by the next call.
 * SE2GPU_ERR_INVALID: a NULL handle or required pointer, npairs / cap / nframes < 1, mp_only != 0 without d_has_mp.
 * SE2GPU_ERR_CAPACITY: cap > 65536 - the vbMatched2 flags of a vocabulary node, one LDS byte per feature of frame b, take
 * `cap` rounded up to 64 bytes of the 64 KiB a workgroup gets without opting in (the transform's own limit is 4096); or
 * npairs > 65535, the pairs being one dimension of a launch. */
int se2gpu_search_by_bow_batch_device(se2gpu_matcher* h,
                                      const se2gpu_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts, int cap,
                                      int nframes,
                                      const int32_t* d_fv_nodes, const int32_t* d_fv_ptr, const int32_t* d_fv_idx,
                                      const int32_t* d_fv_nn,
                                      const uint8_t* d_has_mp,
                                      const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs,
                                      int mp_only, float nnratio, int check_orientation,
                                      int32_t* d_matches12, int32_t* d_nmatches);

/* MapPoint::updateMainKFandDescriptor (src/MapPoint.cpp:228-292 of the reference) for a batch of m map points whose
 * observations lie in the frame arrays se2gpu_orb_extract_batch_device writes (d_kps from f * cap, d_desc from f * cap * 32,
 * d_counts[f]; descriptors 8-byte aligned).  Every pointer is device memory except scale_factors.
 *   d_frame_null   nframes bytes or NULL: 1 = KeyFrame::isNull() (:242)
 *   d_view_pos     nframes * cap * 3 floats or NULL: KeyFrame::mViewMPs[idx] (:287); NULL writes no distances
 *   scale_factors  HOST array of nlevels floats, mvScaleFactors (:286, :291); read during the call, needed with d_view_pos
 *   d_mp_ptr (m + 1), d_obs_frame / d_obs_ftr (nobs each): the observations in CSR form, point p owns entries
 *                  d_mp_ptr[p] .. d_mp_ptr[p + 1] - 1.  ORDER MATTERS: list a point's observations in the order the caller's
 *                  container iterates them (the reference's std::map<PtrKeyFrame, int>, include/se2lam/MapPoint.h:86,
 *                  iterates in the order of the shared pointers' addresses).  On equal medians the earliest observation of the list wins, as `median < bestMedian`
 *                  (:272) lets the first one iterated win; another order can pick another main key frame.
 *   d_prev_main_frame  m ints or NULL: the frame of the point's mMainKF before the call, -1 = none (:280)
 * Per point: an observation is valid when its frame lies in 0..nframes-1, the frame is not null and its feature lies in
 * 0..min(counts, cap)-1; the others are skipped (nothing is indexed outside the arrays whatever they hold; d_mp_ptr values
 * are clamped to 0..nobs and a descending segment is empty).  Over the N valid ones in list order, D[i][j] = 256-bit Hamming
 * distance, median of row i = element (N-1)/2 of the row sorted ascending (self-distance 0 included), main observation =
 * the first i whose median is strictly smaller than every earlier one.
 *   d_info[4p..]       {place of the main observation in the point's list (skipped entries counted), its median, N, changed};
 *                      {-1, 0, 0, 0} and nothing else written when N == 0
 *   d_main_desc[32p..] its descriptor, always (:278);  d_main_frame[p] its frame
 *   changed            bit 0: the frame differs from d_prev_main_frame[p] (or that array is NULL).  Only then (:280 returns
 *                      early otherwise and the old values stay):
 *   d_main_octave[p]   = kps.octave (:285)
 *   d_dist[2p..]       = {mMinDist, mMaxDist} (:290-291): dist = (float)sqrt((double)x*x + (double)y*y + (double)z*z) with a
 *                      correctly rounded FP64 square root, max = dist * scale_factors[octave], min = max /
 *                      scale_factors[nlevels - 1], in float.  An octave outside 0..nlevels-1 leaves them untouched and sets
 *                      bit 1 of changed (with or without d_view_pos).
 * A point's outputs depend on its own list only: not on the batch, its place in it or the run.
 * Asynchronous on the matcher's stream: nothing is read back and nothing waits; se2gpu_matcher_sync waits for it.  The call
 * needs no scratch memory.
 * The argument checks come first and touch neither the handle nor a device:
 * SE2GPU_ERR_INVALID: a NULL handle, d_kps, d_desc, d_counts, d_mp_ptr or output (d_dist only with d_view_pos); nobs > 0
 *   without d_obs_frame / d_obs_ftr; m < 0, nobs < 0, cap < 1, nframes < 1, nlevels < 1; d_view_pos without scale_factors.
 * SE2GPU_ERR_CAPACITY: nlevels > 32 (the factors are kernel arguments); nframes * cap > 2^31 - 1.
 * m == 0 is SE2GPU_OK and launches nothing. */
int se2gpu_mappoint_main_batch_device(se2gpu_matcher* h,
                                      const se2gpu_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts, int cap,
                                      int nframes, const uint8_t* d_frame_null, const float* d_view_pos,
                                      const float* scale_factors, int nlevels,
                                      const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr,
                                      int m, int nobs, const int32_t* d_prev_main_frame,
                                      int32_t* d_info, uint8_t* d_main_desc, int32_t* d_main_frame, int32_t* d_main_octave,
                                      float* d_dist);

/* MapPoint::updateParallax (src/MapPoint.cpp:124-185 of the reference), the rule every MapPoint::addObservation runs, for a
 * batch of m map points.  The sibling of se2gpu_mappoint_main_batch_device: the same frame layout and the same observation
 * CSR (d_mp_ptr, d_obs_frame, d_obs_ftr in the caller's container order).  Every pointer is device memory.
 *   d_kps_un       nframes * cap: keyPointsUn (x, y are read); may be the extractor's d_kps itself
 *   d_counts       nframes
 *   d_frame_Tcw, d_frame_Twc, d_frame_P   nframes x 12 floats each: rows 0-2 (row-major) of Tcw, of cvu::inv(Tcw) and of
 *                  Kcam * Tcw.  The inverse and the projection come from the caller; the camera centre is column 3 of Twc
 *   d_frame_idkf   nframes ints: mIdKF
 *   d_good_prl     m bytes: mbGoodParallax before the call
 *   d_new_frame    m ints: the frame of pKF, the observation just added
 *   fx, lower_depth, upper_depth   Config::fxCam, LOWER_DEPTH, UPPER_DEPTH
 *   d_kf_observed  nframes * cap bytes or NULL, in/out: KeyFrame::hasObservation(idx)
 * Per point p: an entry is valid when its frame lies in 0..nframes-1 and its feature in 0..min(counts, cap)-1; the others
 * are skipped and not counted (a null key frame is NOT skipped: the reference does not skip it here).  N = valid entries.
 *   status 0, nothing done: d_good_prl[p] set, N <= 2 (:125), or no valid entry of d_new_frame[p] (pKF = the first one).
 *   pKF0 = the valid entry with the smallest idkf among those with idkf(pKF) - idkf(entry) <= 6, the first in list order on
 *          equal ids (:129-139).
 *   pKF0's frame is pKF's: status 3 (the reference triangulates a ray against itself, fails the parallax test, age 0).
 *   Otherwise (:142-153) posW = cvu::triangulate(pt0, pt1, P0, P1) - rows in float, one-sided Jacobi in FP64, dehomogenised
 *   in float, as se2gpu_triangulate -, pos0 / pos1 = cvu::se3map, Config::acceptDepth on both depths, cvu::checkParallax
 *   against 0.9994f.
 *   status 1, promoted (:154-177): d_pos[3p..] = posW; (info0, info1) = Track::calcSE3toXYZInfo(pos0, Tcw0, Tcw1) (float
 *          arithmetic in the reference's order, norms, cv::Rodrigues and matrix sums in double, asinf; 3x3 row-major floats);
 *          xyzinfoW = Rcw0^T info0 Rcw0.  For every valid entry e (index into the CSR arrays) d_obs_view[3e..] /
 *          d_obs_info[9e..]: pKF0 gets pos0 / info0, pKF pos1 / info1, every other entry se3map(Tcw_k, posW) and
 *          Rcw_k xyzinfoW Rcw_k^T, except an entry with the idkf of pKF or pKF0, which is left alone (:169).
 *   status 2, abandoned (:182-184): not promoted and idkf(pKF) - idkf(pKF0) >= 6.  With d_kf_observed the byte of every
 *          valid entry is cleared (MapPoint::setNull, :68-78).
 *   status 3: not promoted, younger.
 *   d_status[p], d_pkf0_place[p] (place of pKF0 in the point's list, skipped entries counted, -1 with status 0): always
 *   written.  Nothing else is written for a point that is not promoted.
 * A point's outputs depend on its own list only.  One thread per point, no atomics, no scratch memory.
 * Asynchronous on the matcher's stream: nothing is read back; se2gpu_matcher_sync waits for it.
 * The argument checks come first and touch neither the handle nor a device:
 * SE2GPU_ERR_INVALID: a NULL handle, frame array, d_frame_idkf, d_mp_ptr, d_good_prl, d_new_frame, d_status, d_pkf0_place
 *   or d_pos; nobs > 0 without d_obs_frame / d_obs_ftr / d_obs_view / d_obs_info; m < 0, nobs < 0, cap < 1, nframes < 1.
 * SE2GPU_ERR_CAPACITY: nframes * cap > 2^31 - 1.   m == 0 is SE2GPU_OK and launches nothing. */
int se2gpu_mappoint_parallax_batch_device(se2gpu_matcher* h,
                                          const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap, int nframes,
                                          const float* d_frame_Tcw, const float* d_frame_Twc, const float* d_frame_P,
                                          const int32_t* d_frame_idkf,
                                          const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr,
                                          int m, int nobs, const uint8_t* d_good_prl, const int32_t* d_new_frame,
                                          float fx, float lower_depth, float upper_depth, uint8_t* d_kf_observed,
                                          int32_t* d_status, int32_t* d_pkf0_place, float* d_pos, float* d_obs_view,
                                          float* d_obs_info);

/* The three passes of LocalMapper::findCorrespd (src/LocalMapper.cpp:87-170) for a batch of B new key frames: which feature
 * of the new key frame becomes an observation, with its KeyFrame::mViewMPs[idx] and mViewMPsInfo[idx].  The frame arrays,
 * pose tables and d_kf_observed (required here) are those of se2gpu_mappoint_parallax_batch_device; d_view_pos is the
 * mViewMPs table of se2gpu_mappoint_main_batch_device (nframes * cap * 3 floats).  Every pointer is device memory.
 * Job b:  d_job_prev[b], d_job_new[b]  frame slots of the previous and the new key frame (different, in range; another job
 *                                       is left with kind 0 everywhere).  THE 2 B SLOTS OF A BATCH MUST BE PAIRWISE DISTINCT:
 *                                       a job reads and writes the kf_observed bytes of its two frames, and two jobs that
 *                                       share a frame would do so in no defined order.  The call cannot see the slots (they
 *                                       are device memory) and does not check this; key frames that follow one another (the
 *                                       new one of a job being the previous one of the next) go into successive calls
 *         d_Tcr, d_Trc (B x 12)        mNewKF->Tcr and its inverse, rows 0-2
 *         d_matched12 (B * cap)        vMatched12 as doTriangulate left it, feature i of prev -> feature of new or -1
 *         d_local_pos (B * cap * 3)    localMPs, in the previous key frame
 *         d_match_idx_mp (B * cap)     the row se2gpu_match_projection_device wrote for this key frame (index into the
 *                                       map-point table, -1 = none); needed with pass 2
 * Map-point table (m points): d_mp_main_frame / d_mp_main_ftr / d_mp_main_octave (the main observation), d_mp_normal (m x 3,
 * mNormalVector), d_mp_dist (m x 2, {mMinDist, mMaxDist} as se2gpu_mappoint_main_batch_device writes them).
 * passes: bit 0, 1, 2 = pass 1, 2, 3.
 * First inv[j] = i is built from the matched12 row into d_inv (B * cap ints, work space and output): -1 where no i with
 * i < counts[prev] and matched12[i] in 0..counts[new]-1 points at j, the greatest such i otherwise; d_counts_out[5b + 4]
 * counts the claims beyond the first.  The reference's input is injective after the RANSAC: a non-zero count says it was not.
 * Then one thread per feature j < min(counts[new], cap), the passes in this order, the first that applies wins:
 *   pass 1 (:95-107)   i = inv[j] >= 0 and kf_observed[prev][i]:  view = se3map(Tcr, mViewMPs_prev[i]), info = the second
 *                      output of calcSE3toXYZInfo(mViewMPs_prev[i], I, Tcr).  kind 1, src = i.
 *   pass 2 (:119-141)  kf_observed[new][j] clear on entry and q = match_idx_mp[j] in 0..m-1 with a valid main observation:
 *                      x3d = cvu::triangulate(kps_un[main], kps_un[new][j], P_main, P_new), posNewKF = se3map(Tcw_new, x3d);
 *                      if MapPoint::acceptNewObserve (0.866f, |octave difference| <= 2, min <= dist <= max) and
 *                      lower_depth <= z <= upper_depth: view = posNewKF, info = the first output of
 *                      calcSE3toXYZInfo(posNewKF, Tcw_new, Tcw_main).  kind 2, src = q.
 *   pass 3 (:145-168)  kf_observed[new][j] clear on entry, i = inv[j] >= 0 and kf_observed[prev][i] clear:
 *                      view = se3map(Tcr, local_pos[i]), (info_prev, info) = calcSE3toXYZInfo(local_pos[i], Tcw_prev,
 *                      Tcw_new); d_new_pos_w[3(b cap + j)..] = se3map(Twc_prev, local_pos[i]), d_info_prev[9(b cap + j)..].
 *                      kind 3, src = i.  (vbGoodPrl[i] was decided by doTriangulate; the caller passes it on.)
 * Outputs per (b, j), j < cap: d_kind (byte, 0 = none) and d_src (-1 for kind 0) always; d_view (3 floats) and d_info (9,
 * row-major) for kinds 1-3.  d_counts_out[5b + k], k = 0..3: features of kind k.  kf_observed[new][j] is set for kinds 1-3
 * and kf_observed[prev][i] for kind 3; a thread writes only bytes it owns.  Integer atomics only: with pairwise distinct
 * frame slots the outputs are the same in every run and wherever a job stands in the batch.
 * A point abandoned by updateParallax inside pass 1 frees its feature before MatchByProjection looks at it
 * (MapPoint.cpp:73-74, ORBmatcher.cpp:417), so the faithful order is: passes = 1, se2gpu_mappoint_parallax_batch_device
 * over the tracked points that are not yet good parallax, the main descriptors, MatchByProjection, passes = 6.
 * passes = 7 in one call is for callers with no such point pending.
 * Asynchronous on the matcher's stream (two memsets, two launches); se2gpu_matcher_sync waits for it.
 * The argument checks come first and touch neither the handle nor a device:
 * SE2GPU_ERR_INVALID: a NULL handle, frame array, d_kf_observed, d_job_prev, d_job_new, d_Tcr, d_matched12, d_inv or
 *   output; d_view_pos / d_Trc NULL with pass 1, d_match_idx_mp (or, with m > 0, the map-point table) NULL with pass 2,
 *   d_local_pos / d_new_pos_w / d_info_prev NULL with pass 3; B < 0, m < 0, cap < 1, nframes < 1; passes outside 1..7.
 * SE2GPU_ERR_CAPACITY: nframes * cap or B * cap > 2^31 - 1, B > 65535.   B == 0 is SE2GPU_OK and launches nothing. */
int se2gpu_kf_correspd_batch_device(se2gpu_matcher* h,
                                    const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap, int nframes,
                                    const float* d_frame_Tcw, const float* d_frame_Twc, const float* d_frame_P,
                                    uint8_t* d_kf_observed, const float* d_view_pos,
                                    const int32_t* d_job_prev, const int32_t* d_job_new, const float* d_Tcr,
                                    const float* d_Trc, const int32_t* d_matched12, const float* d_local_pos,
                                    const int32_t* d_match_idx_mp, int B,
                                    const int32_t* d_mp_main_frame, const int32_t* d_mp_main_ftr,
                                    const int32_t* d_mp_main_octave, const float* d_mp_normal, const float* d_mp_dist, int m,
                                    float fx, float lower_depth, float upper_depth, int passes,
                                    int32_t* d_inv, uint8_t* d_kind, int32_t* d_src, float* d_view, float* d_info,
                                    float* d_new_pos_w, float* d_info_prev, int32_t* d_counts_out);

/* The map's bookkeeping for a batch of B new key frames, and for pruned ones: what LocalMapper::findCorrespd's addObservation /
 * setViewMP / insertMP calls (src/LocalMapper.cpp:95-168), MapPoint::addObservation's normal vector (src/MapPoint.cpp:104-122) and
 * the erasures of KeyFrame::setNull / MapPoint::eraseObservation / MapPoint::setNull (src/KeyFrame.cpp:100-113,
 * src/MapPoint.cpp:54-101) do to the observation table every other call reads.  It writes a NEW table (CSR and entry rows) of
 * capacities m_cap / nobs_cap from the old one and the rows se2gpu_kf_correspd_batch_device left, and updates the per-point and
 * per-feature tables in place.  Every pointer is device memory.
 *   d_counts, cap, nframes, d_frame_null (nframes bytes or NULL)   the frame slots; a set byte = KeyFrame::isNull()
 *   d_mp_ptr (m_cap + 1), d_obs_frame, d_obs_ftr (nobs_cap), d_obs_view (nobs_cap x 3), d_obs_info (nobs_cap x 9)   the old table;
 *       the two entry rows and their new counterparts are optional, all four or none
 *   d_sizes_in   {m_old, nobs_old} in DEVICE memory, clamped to 0..m_cap and 0..nobs_cap: d_sizes_out + 1 of the call before,
 *       so that calls follow one another without the host knowing the sizes (the two may be the same buffer)
 *   d_job_prev, d_job_new (B), d_kind, d_src, d_view, d_info, d_new_pos_w, d_info_prev (B * cap rows, by the new key frame's
 *       feature j), d_local_pos (by the previous key frame's feature)   as se2gpu_kf_correspd_batch_device takes / leaves them
 *   d_good_prl_row (B * cap bytes)   mvbGoodPrl of se2gpu_track_frames_batch_device, by the previous key frame's feature
 *   kinds   bit k (1..3) = apply the rows of kind k, so the faithful order (passes = 1, apply, parallax, ..., passes = 6, apply)
 *       can use one row buffer
 *   d_parallax_status (m_cap ints or NULL)   d_status of se2gpu_mappoint_parallax_batch_device: 2 counts as a null point here
 *   in place, per point (m_cap): d_pos (x 3), d_good_prl, d_mp_null (bytes), d_mp_normal (x 3)
 *   in place, per feature (nframes * cap): d_ftr_mp (mDualObservations: the point's slot or -1), d_kf_observed (bytes),
 *       d_view_pos (x 3), d_view_info (x 9)
 *   out: d_mp_ptr_new, d_obs_frame_new, d_obs_ftr_new, d_obs_view_new, d_obs_info_new (not the old arrays); d_new_frame (m_cap):
 *       the frame slot of the entry this call appended to the point (the last job's if several did), -1 for none - what
 *       se2gpu_mappoint_parallax_batch_device takes as d_new_frame; d_sizes_out (SE2GPU_MAP_APPLY_NSIZES ints, below);
 *       d_job_counts (B x 6): {1 if the job was skipped, rows of kind 1, 2, 3 applied, rows skipped, duplicate claims}
 *   d_ws   se2gpu_map_apply_ws_bytes(B, cap, m_cap, nobs_cap) bytes, 16-byte aligned, no initialisation needed; -1 on sizes
 *       the call would refuse
 * The rules, in this order:
 * 1. Erase first, on the state at entry.  An old entry (f, k) of point p < m_old is dropped when
 *      - it fails the entry rule of se2lam_amd/obs_table.h (f outside 0..nframes-1 or k outside 0..min(counts[f], cap)-1);
 *      - its point is null or has parallax status 2 - MapPoint::setNull, MapPoint.cpp:68-78: pKF->eraseObservation(idx) makes
 *        ftr_mp[f][k] = -1 and kf_observed[f][k] = 0, mbNull = true and mbGoodParallax = false (:69-70);
 *      - its frame is null - KeyFrame::setNull, KeyFrame.cpp:101-104: pMP->eraseObservation(pThis) for each of its points.  With
 *        size = the point's entries left after this erase (entries that fail the entry rule never counted), size > 0 updates
 *        mNormalVector = (mNormalVector * (float)(size + 1) - normPos) * (1.f / (float)size), normPos = viewPos * (1.f /
 *        cv::norm(viewPos)), viewPos = view_pos[f][k] (MapPoint.cpp:89-90, :98-99), in list order.
 *    Every null frame's ftr_mp row becomes -1 and its kf_observed row 0 (KeyFrame.cpp:110-111).  A point that was not null and is
 *    left without entries becomes null with good_prl cleared (MapPoint.cpp:93-94, :56-57).  Kept entries keep their order.
 * 2. Rows of kind 1 and 2 append one entry (job_new[b], j) to point p = ftr_mp[job_prev[b]][src] as it was at entry (kind 1,
 *    pPrefKF->getObservation(i), LocalMapper.cpp:97) or p = src (kind 2, :122), after the kept entries; several jobs that add
 *    to one point append in ascending job index.  The call writes view_pos / view_info of the feature (setViewMP, :103, :138),
 *    ftr_mp = p and kf_observed = 1 (KeyFrame::addObservation, KeyFrame.cpp:199-200), the entry's rows, and mNormalVector =
 *    (mNormalVector * (float)oldObsSize + newNorm) * (1.f / (float)(oldObsSize + 1)) with oldObsSize = the list's length before
 *    the append (MapPoint.cpp:107, :115-117).  A row is skipped, counted, its kf_observed byte cleared and nothing else written
 *    when it names no point or one outside 0..m_old-1; a point that is null after rule 1 (KeyFrame::addObservation returns,
 *    KeyFrame.cpp:197); a point that keeps an entry of that frame (std::map::insert keeps the old one, MapPoint.cpp:108).  If
 *    several features of one job name one point the greatest j wins, whatever becomes of it; the others are skipped and also
 *    counted as duplicate claims.
 * 3. Rows of kind 3 create a point (LocalMapper.cpp:145-168).  src must lie in 0..min(counts[prev], cap)-1 (else skipped);
 *    of several rows with one src the greatest j wins (the others: skipped, duplicate).  Slot = m_old + the winners of earlier
 *    jobs + the row's rank among its job's winners by ascending src: the loop at :145 runs over the previous key frame's features
 *    and MapPoint::mId grows in that order.  Entries (prev, src) then (new, j) (:160-161); pos = new_pos_w, good_prl =
 *    good_prl_row[b][src] (:158), mp_null = 0, the normal from the two appends starting at zero; view_pos[prev][src] =
 *    local_pos[b][src], view_info[prev][src] = info_prev[b][j] (:156); the new key frame's feature as in rule 2; ftr_mp and
 *    kf_observed of both features (:162-163).
 * 4. Padding: mp_ptr_new[p] = nobs_new for p = m_new..m_cap; the point slots from m_new on are null, not good-parallax, with
 *    new_frame = -1.  The table can therefore be handed to every consumer with m = m_cap and nobs = nobs_cap.
 * 5. Capacity: m_new > m_cap or nobs_new > nobs_cap gives status 2 in d_sizes_out; the sizes and counts say what was needed,
 *    nothing in place has been modified and the new table is undefined.
 * 6. The 2 B frame slots of a batch are pairwise distinct, as for se2gpu_kf_correspd_batch_device.  A job with a slot out of
 *    range, prev == new or a null frame is skipped (d_job_counts[6b] = 1, its rows are not looked at).  B == 0 is a pure erase
 *    pass: Map::pruneRedundantKF's KeyFrame::setNull, or the points se2gpu_mappoint_parallax_batch_device abandoned.
 * Asynchronous on the matcher's stream (memsets and launches; nothing allocated, read back or waited for); every output word
 * is the same in every run: integer atomicMax picks a claim's winner, integer atomicAdd only sums counters, places come from
 * prefix sums.  The argument checks come first and touch neither the handle nor a device:
 * SE2GPU_ERR_INVALID: a NULL handle or required pointer (optional: d_frame_null, the four entry rows together,
 *   d_parallax_status; with B == 0 the job arrays and d_job_counts; without bit 3 of kinds d_new_pos_w, d_info_prev, d_local_pos,
 *   d_good_prl_row); B < 0, m_cap < 0, nobs_cap < 0, cap < 1, nframes < 1; kinds with bits outside 1..3; a new array equal to
 *   its old one; d_ws not 16-byte aligned.
 * SE2GPU_ERR_CAPACITY: nframes * cap > 2^31 - 1; B > 65535, B * m_cap > 2^31 - 1, m_cap + B * cap or nobs_cap + 2 B cap + 1 not
 *   below 2^31 - 1; ws_bytes too small.   B == 0 with m_cap == 0 (no job, and no point slot to erase anything from) is
 *   SE2GPU_OK, launches nothing and writes nothing: d_sizes_out and d_mp_ptr_new are NOT written either, so such a call is
 *   no link of a chain (a later call must not take its d_sizes_in from it).   SE2GPU_ERR_NO_DEVICE after all of these. */
enum { SE2GPU_MAP_APPLY_STATUS = 0,   /* 0 done, 2 capacity */
       SE2GPU_MAP_APPLY_M_NEW, SE2GPU_MAP_APPLY_NOBS_NEW, SE2GPU_MAP_APPLY_ADDED, SE2GPU_MAP_APPLY_ERASED,
       SE2GPU_MAP_APPLY_CREATED, SE2GPU_MAP_APPLY_NULLED, SE2GPU_MAP_APPLY_SKIPPED, SE2GPU_MAP_APPLY_DUP,
       SE2GPU_MAP_APPLY_NSIZES };
long long se2gpu_map_apply_ws_bytes(int B, int cap, int m_cap, int nobs_cap);
int se2gpu_map_apply_batch_device(se2gpu_matcher* h,
                                  const int32_t* d_counts, int cap, int nframes, const uint8_t* d_frame_null,
                                  const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr,
                                  const float* d_obs_view, const float* d_obs_info,
                                  const int32_t* d_sizes_in, int m_cap, int nobs_cap,
                                  const int32_t* d_job_prev, const int32_t* d_job_new, int B,
                                  const uint8_t* d_kind, const int32_t* d_src, const float* d_view, const float* d_info,
                                  const float* d_new_pos_w, const float* d_info_prev, const float* d_local_pos,
                                  const uint8_t* d_good_prl_row, int kinds, const int32_t* d_parallax_status,
                                  float* d_pos, uint8_t* d_good_prl, uint8_t* d_mp_null, float* d_mp_normal,
                                  int32_t* d_ftr_mp, uint8_t* d_kf_observed, float* d_view_pos, float* d_view_info,
                                  int32_t* d_mp_ptr_new, int32_t* d_obs_frame_new, int32_t* d_obs_ftr_new,
                                  float* d_obs_view_new, float* d_obs_info_new, int32_t* d_new_frame,
                                  int32_t* d_sizes_out, int32_t* d_job_counts, void* d_ws, long long ws_bytes);

/* Covisibility: Map::compareViewMPs (src/Map.cpp:354-400 of the reference, both overloads) for batches, on the observation
 * CSR of se2gpu_mappoint_parallax_batch_device.  The observation sets live in a caller-supplied bit matrix d_bits of
 * (nframes + 2) rows of W = ceil(m / 64) 64-bit words, bit p & 63 of word p / 64 = point p:
 *   row f < nframes   key frame slot f's mObservations over the m points
 *   row nframes       point is not null               (what getAllObsMPs(false) keeps, KeyFrame.cpp:152)
 *   row nframes + 1   not null and good parallax      (what getAllObsMPs() keeps: checkParallax defaults to true, KeyFrame.h:69)
 * Bits past m are zero.  se2gpu_covis_bits_words (host only, no device) returns the number of words, (nframes + 2) * W, or
 * -1 with nframes < 1 or m < 0.
 *
 * se2gpu_covis_build_device fills d_bits and d_size_obs from the CSR.  Every pointer is device memory.
 *   THE CSR MUST DESCRIBE THE KEY FRAME'S SIDE: point p lists frame f iff pKF_f->mObservations holds p.  compareViewMPs reads
 *   only that side (getAllObsMPs, hasObservation(pMP), getSizeObsMP are KeyFrame members), never MapPoint::mObservations.
 *   d_mp_null    m bytes or NULL (none is null): MapPoint::isNull()
 *   d_good_prl   m bytes or NULL (all good): MapPoint::isGoodPrl()
 *   Bit (f, p) is set iff point p's list holds at least one valid entry of frame f.  Validity is the rule of
 *   se2gpu_mappoint_parallax_batch_device: the frame lies in 0..nframes-1 and the feature in 0..min(counts, cap)-1; a null key
 *   frame is not skipped.  d_mp_ptr values are clamped to 0..nobs and a descending segment is empty.  A frame that appears
 *   twice in one list counts once.
 *   d_size_obs[f] (nframes ints) = the popcount of row f = KeyFrame::getSizeObsMP() (KeyFrame.cpp:122-125): mObservations.size()
 *   counts null points too.
 *   A memset of the key-frame rows, one thread per point (64-bit integer atomicOr; the two point rows by ballot), one wave per
 *   row for the sizes: the memset is inside the call, so a second build gives the same bits.  m == 0 launches nothing and
 *   leaves d_size_obs alone (se2gpu_covis_pairs_device counts the rows itself and needs no d_size_obs).
 *
 * se2gpu_covis_pairs_device: Point2f Map::compareViewMPs(pKF1, pKF2, spMPs) (:354-369) for npairs pairs of slots
 * (d_pair_a[p], d_pair_b[p]) = (pKF1, pKF2), one wave per pair.
 *   d_pair_out[4p..]   {n_same, size_a, size_b, flags}: n_same = popcount(row a & row b & not-null row) (:358-365; the null
 *                      points are dropped from the numerator and not from the sizes), size = popcount of the row
 *   d_pair_ratio[2p..] {(float)n_same / (float)size_a, (float)n_same / (float)size_b} (:367-368), one IEEE division each;
 *                      0 / 0 is NaN as in the reference
 *   flags bit 0        (float)n_same > ratio_f * (float)size_a: Map::updateCovisibility's test with 0.3f (:794), one float
 *                      multiply and a compare in float
 *   flags bit 1        (double)n_same > ratio_d * (double)size_a: Localizer::UpdateCovisKFCurr's with 0.1 (Localizer.cpp:683)
 *   A pair with a slot outside 0..nframes-1 gets {-1, 0, 0, 0}; its ratios and its list are left untouched.  a == b is legal.
 *   With m == 0 every in-range pair gets {0, 0, 0, 0} and NaN ratios.  A pair's outputs depend on that pair alone.
 *   Optional list, with d_common != NULL (then d_counts, cap, d_mp_ptr, d_obs_frame, d_obs_ftr, nobs of the build are
 *   required, whatever list_cap is; without d_common they are not read and may be NULL / 0, and list_cap is ignored):
 *   d_common[3 (p * list_cap + i)..] = {point, e_a, e_b} for the first list_cap common points in ascending point index - the
 *   spMPs GlobalMapper::CreateFeatEdge turns into vPtrMPs (GlobalMapper.cpp:741-750).  e_a / e_b are the CSR entry indices of
 *   the first valid entry of frames a / b in that point's list (-1 if the CSR no longer holds one): gather mp_xyz, m_z and
 *   m_info for se2gpu_feat_edge_batch from d_obs_view / d_obs_info with them, or hand d_pair_out and d_common to
 *   se2gpu_feat_edge_batch_device, which does that on the device.  Truncation shows as n_same > list_cap; entries
 *   from min(n_same, list_cap) on are left untouched.  The order is fixed by a prefix sum over the wave, without atomics.
 *
 * se2gpu_covis_refset_device: double Map::compareViewMPs(pKFNow, spKFsRef, spMPsRet, k) (:373-400) for njobs jobs, one wave
 * per job: key frame slot d_job_kf[j] against the slots d_ref_idx[d_ref_ptr[j] .. d_ref_ptr[j + 1] - 1] (d_ref_ptr: njobs + 1
 * ints, clamped to 0..nref, a descending segment is empty).
 *   all = popcount(row kf & good-parallax row) (:376); cnt = the points of that set observed by at least k of the listed
 *   reference frames (:381-396).  Entries outside 0..nframes-1 are skipped.  A SLOT LISTED TWICE COUNTS TWICE: the reference's
 *   std::set has no duplicates, and keeping the list free of them is the caller's duty.  The job's own slot counts if listed.
 *   d_job_out[3j..] = {cnt, all, redundant}; d_job_ratio[j] = (double)cnt * 1.0 / (double)all (:398), -1.0 with all == 0
 *   (:377-379); redundant = ratio >= thresh, Map::pruneRedundantKF's test with 0.8 (:196), 0 with all == 0.
 *   A job slot out of range gives {-1, 0, 0} and leaves its ratio untouched.  k in 1..7: the count is kept in three bit planes.
 *
 * All three are asynchronous on the matcher's stream: nothing is read back; se2gpu_matcher_sync waits for them.  No scratch
 * memory.  Integer atomics only: the same words in every run.
 * The argument checks come first and touch neither the handle nor a device; se2gpu_last_error names the argument:
 * SE2GPU_ERR_INVALID: a NULL handle, d_bits, required array (d_counts, d_mp_ptr; d_obs_frame / d_obs_ftr with nobs > 0;
 *   d_pair_a, d_pair_b; d_job_kf, d_ref_ptr; d_ref_idx with nref > 0) or output; m < 0, nobs < 0, npairs < 0, njobs < 0,
 *   nref < 0, nframes < 1, cap < 1 (where the CSR is read), list_cap < 0; d_common without the CSR arrays.
 * SE2GPU_ERR_CAPACITY: (nframes + 2) * W > 2^31 - 1; nframes * cap > 2^31 - 1 (where the CSR is read); npairs or njobs >
 *   2^26 - 1 = 67108863 (64 threads each, and a launch's threads stay below 2^32); k outside 1..7.
 * npairs == 0, njobs == 0 and m == 0 at build are SE2GPU_OK and launch nothing. */
long long se2gpu_covis_bits_words(int nframes, int m);
int se2gpu_covis_build_device(se2gpu_matcher* h, const int32_t* d_counts, int cap, int nframes,
                              const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr, int m, int nobs,
                              const uint8_t* d_mp_null, const uint8_t* d_good_prl, uint64_t* d_bits, int32_t* d_size_obs);
int se2gpu_covis_pairs_device(se2gpu_matcher* h, const uint64_t* d_bits, int nframes, int m,
                              const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs, float ratio_f, double ratio_d,
                              int32_t* d_pair_out, float* d_pair_ratio,
                              int32_t* d_common, int list_cap, const int32_t* d_counts, int cap,
                              const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr, int nobs);
int se2gpu_covis_refset_device(se2gpu_matcher* h, const uint64_t* d_bits, int nframes, int m,
                               const int32_t* d_job_kf, const int32_t* d_ref_ptr, const int32_t* d_ref_idx, int nref, int njobs,
                               int k, double thresh, int32_t* d_job_out, double* d_job_ratio);

/* Local window: the covisibility graph KeyFrame::mCovisibleKFs as a bit matrix in device memory, the calls that maintain it,
 * and Map::updateLocalGraph (src/Map.cpp:285-331 of the reference) on it for batches of current key frames.
 *
 * d_adj is supplied by the caller and zeroed by the caller once: nframes rows of WF = ceil(nframes / 64) 64-bit words, bit
 * b & 63 of word b / 64 of row a = "slot b is in slot a's mCovisibleKFs".  It is directed: the reference's set is per key
 * frame, and only the callers of addCovisibleKF keep it symmetric.  Bits past nframes are zero.  se2gpu_covis_adj_words (host
 * only, no device) returns the number of words, nframes * WF, or -1 with nframes < 1.
 *
 * se2gpu_covis_connect_device: addCovisibleKF in both directions, one thread per pair (64-bit integer atomicOr), for every
 * pair (d_pair_a[p], d_pair_b[p]) whose two slots lie in 0..nframes-1 and for which
 *   d_pair_out == NULL                    the unconditional links of LocalMapper.cpp:66-67, Map.cpp:233-234 and :337-338, or
 *   d_pair_out[4p + 3] & flag_mask != 0   d_pair_out as se2gpu_covis_pairs_device wrote it; flag_mask = 1 is Map.cpp:794-797.
 *   a == b sets the one diagonal bit.  No bit is ever cleared.  Pairs out of range are skipped.
 *
 * se2gpu_covis_disconnect_device: the covisibility part of KeyFrame::setNull (KeyFrame.cpp:106-114) for the nslots slots of
 * d_slots.  For every listed slot s in range, bit (b, s) is cleared for every b in row s, then row s is zeroed.  A key frame
 * that lists s while s does not list it keeps s, as in the reference.  Slots out of range are skipped.
 *   Two launches on the stream: the first clears the bits (b, s) read from the rows as they stand (one wave per listed slot,
 *   64-bit integer atomicAnd), the second zeroes the listed rows.  SLOTS LISTED TWICE, AND TWO LISTED SLOTS THAT NAME EACH
 *   OTHER, GIVE THE RESULT OF THE REFERENCE'S CALLS IN ANY ORDER: a setNull(s) changes other rows only in column s, so before
 *   its own turn the row of a listed slot s can lose only bits in the columns of other listed slots s' - and those bits decide
 *   only whether (s', s) is cleared, a bit of row s', which ends as zero whatever the order.  For an unlisted b the bit (b, s)
 *   is cleared iff b was in row s at the start, in every order; the first launch computes exactly that, and clearing is
 *   idempotent.
 *
 * se2gpu_local_window_batch_device: Map.cpp:285-331 for njobs current key frames d_job_kf[j], one workgroup per job.
 *   d_bits_kf     the d_bits of se2gpu_covis_build_device (nframes + 2 rows of W = ceil(m / 64) words) built from the key
 *                 frame's side; serves KeyFrame::getAllObsMPs(false): key-frame row AND the not-null row nframes (:313)
 *   d_bits_mp     a second such matrix built from the CSR of the points' own side, MapPoint::mObservations, which
 *                 getObservations() reads (:320); only its rows 0..nframes-1 are read.  WHERE THE TWO SIDES AGREE, AS THEY DO
 *                 IN A CONSISTENT MAP, PASS THE SAME POINTER TWICE.
 *   d_frame_null  nframes bytes or NULL (none is null): MapPoint::getObservations skips null key frames (MapPoint.cpp:216)
 *   d_kf_order, d_mp_order   nframes / m ints or NULL, read only for the lists (below)
 *   search_level  3 in the reference (:299); any value >= 0
 *   Per job, with cur = d_job_kf[j] in 0..nframes-1:
 *   local   {cur}, then search_level times the union with the adjacency rows of all members AS THE SET STOOD AT THE START OF
 *           THAT ROUND (:300-308 copies the set before it walks it).  Only the members found in the round before are expanded,
 *           which is the same thing, and the rounds stop when one finds nothing.  A null key frame is not skipped (the
 *           reference does not skip it).  Adjacency bits past nframes are ignored.
 *   points  the OR of the d_bits_kf rows of the local key frames, AND the not-null row (:310-315); bits past m are ignored
 *   ref     every slot f that is not local, not d_frame_null[f], and whose d_bits_mp row meets the point set (:317-326)
 *   n_obs   the sum of popcount(d_bits_mp row f & points) over the f of local and ref that are not d_frame_null[f]: the number
 *           of EdgeSE2XYZ Map::loadLocalGraph creates (:1005-1051), to size the graph and to judge whether a window fits the
 *           resident path before it is loaded.  It saturates at 2^31 - 1.
 *   d_win_kf   njobs * 2 * WF words: row 2j = local, row 2j + 1 = ref, as bits over the slots
 *   d_win_mp   njobs * W words: the point set
 *   d_win_out  d_win_out[4j..] = {n_local, n_ref, n_mp, n_obs}
 *   A job slot out of range gives {-1, 0, 0, 0}; its rows and lists are left untouched.  m == 0 still runs the hops; the point
 *   and ref sets are empty.  A job's outputs depend on that job alone, and every call gives the same words in every run.
 *   Optional lists: d_local_list and d_ref_list (njobs * kf_list_cap ints each, either may be NULL), d_mp_list (njobs *
 *   mp_list_cap ints or NULL) hold the members in ascending position of d_kf_order / d_mp_order: each a permutation that lists
 *   the slots / points by ascending mIdKF / mId, the order of the reference's IdLessThan sets and so of mLocalGraphKFs, mRefKFs
 *   and mLocalGraphMPs.  NULL means index order; entries out of range are skipped.  Truncation shows as a count above the cap;
 *   entries from min(count, cap) on are left untouched.  The order comes from a prefix sum over the workgroup, without atomics.
 *
 * All three calls are asynchronous on the matcher's stream; se2gpu_matcher_sync waits for them.  Integers only: no floating
 * point, no scratch memory, integer atomics only.  Every index read from an array (a slot, an order entry, a set bit of a
 * tail word) is checked before it is used.
 * The argument checks come first and touch neither the handle nor a device; se2gpu_last_error names the argument:
 * SE2GPU_ERR_INVALID: a NULL handle, d_adj, d_pair_a, d_pair_b, d_slots, d_bits_kf, d_bits_mp, d_job_kf, d_win_kf, d_win_mp or
 *   d_win_out; nframes < 1, m < 0, npairs < 0, nslots < 0, njobs < 0, search_level < 0, kf_list_cap < 0, mp_list_cap < 0.
 * SE2GPU_ERR_CAPACITY: nframes > SE2GPU_LOCAL_WINDOW_MAX_FRAMES = 4096 (the rows of a window and its member list are held in
 *   LDS; it holds for the upkeep calls too, a d_adj the window call cannot read being of no use); (nframes + 2) * W > 2^31 - 1
 *   as for the covisibility calls (nframes = 4096 admits m up to 33538048); npairs > 2^31 - 256; nslots or njobs > 2^24 - 1 =
 *   16777215 (a launch's threads stay below 2^32).
 * npairs == 0, nslots == 0 and njobs == 0 are SE2GPU_OK and launch nothing. */
#define SE2GPU_LOCAL_WINDOW_MAX_FRAMES 4096
long long se2gpu_covis_adj_words(int nframes);
int se2gpu_covis_connect_device(se2gpu_matcher* h, uint64_t* d_adj, int nframes, const int32_t* d_pair_a,
                                const int32_t* d_pair_b, int npairs, const int32_t* d_pair_out, int flag_mask);
int se2gpu_covis_disconnect_device(se2gpu_matcher* h, uint64_t* d_adj, int nframes, const int32_t* d_slots, int nslots);
int se2gpu_local_window_batch_device(se2gpu_matcher* h, const uint64_t* d_bits_kf, const uint64_t* d_bits_mp, int nframes, int m,
                                     const uint64_t* d_adj, const uint8_t* d_frame_null, const int32_t* d_job_kf, int njobs,
                                     int search_level, const int32_t* d_kf_order, const int32_t* d_mp_order,
                                     uint64_t* d_win_kf, uint64_t* d_win_mp, int32_t* d_win_out,
                                     int32_t* d_local_list, int32_t* d_ref_list, int kf_list_cap,
                                     int32_t* d_mp_list, int mp_list_cap);

/* Local bundle adjustment on the tables where they lie in device memory: Map::loadLocalGraph (src/Map.cpp:891-1053 of the
 * reference) on the lists se2gpu_local_window_batch_device wrote, chained to the one-workgroup-per-window solver that
 * se2gpu_ba_optimize_batch uses for resident batches.  Every array pointer is device memory unless marked host.  Asynchronous
 * on the matcher's stream (three launches: gather, solve, finish): nothing is allocated, nothing uploaded besides kernel
 * arguments, nothing read back and nothing waited for; se2gpu_matcher_sync waits for it.
 * The window, as se2gpu_local_window_batch_device wrote it: d_job_kf (njobs slots), d_win_out ({n_local, n_ref, n_mp, n_obs}
 *   per job), d_local_list / d_ref_list (stride kf_list_cap), d_mp_list (stride mp_list_cap).  All three lists are required.
 * Frame tables (nframes slots): d_frame_id (KeyFrame::id, which the fixed rule reads - not mIdKF); d_frame_Twb (3 floats: Se2
 *   Twb); d_frame_Tcw (12 floats: rows 0-2 of Tcw, the table of se2gpu_mappoint_parallax_batch_device; Rcw is its 3 x 3 block);
 *   d_frame_null (bytes, may be NULL: none is null); preOdomFromSelf as d_odo_to (the slot of .first, or -1), d_odo_meas (3
 *   doubles) and d_odo_cov (9 doubles, row-major) - all three NULL means no odometry edges.
 * Feature tables: d_kps_un (nframes x cap key points: x, y and octave are read), d_counts (nframes), cap, d_view_pos (nframes x
 *   cap x 3 floats, mViewMPs); level_sigma2 is a HOST array of nlevels <= 32 floats (mvLevelSigma2), passed as kernel arguments.
 * Point tables: d_pos (m x 3 floats) and the observation CSR of the points' own side (MapPoint::mObservations, the side d_bits_mp
 *   was built from): d_mp_ptr (m + 1), d_obs_frame, d_obs_ftr (nobs), read by the entry and segment rules of obs_table.h.
 * Configuration (host): fx, cx, cy (Config::Kcam; addCamPara uses fx for both axes); Tbc12 (HOST, 12 doubles: rotation row-major,
 *   translation); huber_delta (Config::TH_HUBER); xrot_info, z_info (PLANEMOTION_XROT_INFO / _Z_INFO; their reciprocals are
 *   rounded to float as :1043-1044 do); iters (1..64); mode (SE2GPU_BA_LM / SE2GPU_BA_GN); max_local, max_ref, max_mp, max_obs:
 *   the sizes the workspace and the launch are cut for.
 * The gather, one workgroup per job, writes the window's graph into the job's slice of d_ws:
 *   vertices  local key frame i -> vertex i, reference key frame i -> n_local + i (:925, :966), map point i -> landmark i
 *   fixed     a reference key frame always (:969); a local one when its id == 1, and with n_ref == 0 the local one(s) with the
 *             least id (:899-927)
 *   poses     doubles converted from the float Twb, the heading normalised as g2o::SE2's constructor does (:929)
 *   odometry  (:935-956) for the local key frames i in order: an edge (i, vertex of d_odo_to[slot]) when that target is a slot
 *             in range, a LOCAL member and not null; info = cov^-1 by the closed-form cofactor inverse se2gpu_ba_load_local_graph
 *             uses.  An edge's place comes from a prefix sum over the workgroup.
 *   landmarks (:980-1051) all n_mp points of d_mp_list in list order, each with its start position d_pos.  A point's edges are
 *             the entries of its CSR list, in list order, that are valid by the entry rule with d_frame_null (null observers
 *             are skipped, :995), whose frame is a member of either list (:1021), and that are the first valid entry of that
 *             frame in the list (getObservations() is a std::set: a frame listed twice counts once, as in
 *             se2gpu_covis_build_device).  Per edge: e_kf, e_uv = keyPointsUn[ftr].pt, e_info by :1024-1049 with sigma2 =
 *             level_sigma2[octave]; an octave outside 0..nlevels-1 skips the edge (its frame stays taken) and sets bit 0 of
 *             the job's flag word.  lm_ptr comes from a prefix sum: the edge order is the same in every run.
 *             checkAssociationErr (:998) compares the two sides of the pointer graph (the key frame's observation of the point
 *             against the point's of the key frame); A ONE-SIDED CSR CANNOT EXPRESS IT, and it is not evaluated.
 *   The information arithmetic is the text k_edge_information runs (csrc/edge_information.h); the two translation units differ in
 *   their contraction setting, so the values agree with se2gpu_ba_edge_information to rounding, not to the bit.
 * d_status[j], the first that applies:
 *   1  the job slot is outside 0..nframes-1, d_win_out[4j] < 0, or a list names a slot / point outside its table: nothing else
 *      but the job's (zero) counts is written
 *   2  does not fit: n_local > min(kf_list_cap, max_local), n_ref > min(kf_list_cap, max_ref), n_mp > min(mp_list_cap, max_mp),
 *      edges > max_obs, more than 64 free key frames (the resident kernel's 192 unknowns), or an odometry self loop
 *      (d_odo_to[slot] == slot of a local key frame: the resident kernel does not take self loops)
 *   3  a local key frame of the window is null: not run.  The reference leaves such a key frame without a vertex (:922) and its
 *      minKFid start (:904) reads a key frame it then skips; the call refuses the window instead of restating that.  A mapper
 *      disconnects null key frames first (se2gpu_covis_disconnect_device), so that no window holds one.
 *   4  a landmark with more than 64 edges (the resident kernel's limit); decided by the gather, the solver is not started
 *   5  nothing to optimise: no free key frame, or no edge at all.  The outputs are the start values.
 *   0  gathered and run;  6  run, and a pose or landmark came out non-finite
 *   Statuses 2-4 write the job's counts as far as they were taken (and scratch); 0 and 5 the whole graph.
 * The solve is one launch of njobs workgroups of the widest of 512 / 256 / 128 threads whose LDS holds a window of max_local +
 * max_ref key frames, min(max_local, 64) of them free; a workgroup whose status is not 0 returns at once.
 * Outputs, per job with status 0 (5: the start values): d_kf_out (njobs x (max_local + max_ref) x 3 doubles, local then
 * reference key frames), d_mp_out (njobs x max_mp x 3 doubles); rows past the job's counts and the rows of other statuses are
 * left untouched.  d_stats (per job, may be NULL): filled from the controller block for status 0 / 6, zero otherwise.
 * d_info[8j..] = {n_pose, n_free, n_lm, n_edge, n_odo, entries of the window's points that became no edge, flag bits, 0}.
 * WRITE-BACK IS THE CALLER'S: the call does not write into d_frame_Twb or d_pos.  Windows of a batch overlap, and the
 * write-back of Map::optimizeLocalGraph (:754-783) for overlapping windows has no defined order.
 * A job's words depend on that job alone: no atomic counter, the same in every run and wherever the job stands in the batch.
 * d_ws: se2gpu_local_ba_ws_bytes(njobs, max_local, max_ref, max_mp, max_obs) bytes supplied by the caller, 16-byte aligned, no
 * initialisation needed; -1 on arguments the call would refuse.  se2gpu_local_ba_ws_layout writes, for the
 * SE2GPU_LOCAL_BA_WS_ARRAYS gathered arrays, the byte offset of job 0's slice and the stride from job to job (n >= that many;
 * SE2GPU_ERR_INVALID otherwise or on those arguments): counts (8 ints, d_info's words), fixed (bytes), poses (x 3 doubles), o_i,
 * o_j (ints), o_meas (x 3), o_info (x 9), lm_ptr (n_lm + 1 ints), e_kf (ints), e_uv (x 2), e_info (x 3: xx, xy, yy), landmarks
 * (x 3) - poses and landmarks are the start values, kept apart from the solver's buffers; valid after the call for the jobs of
 * status 0, 5 and 6.  Both helpers are host only and touch no device.
 * The argument checks come first and touch neither the handle nor a device; se2gpu_last_error names the argument:
 * SE2GPU_ERR_INVALID: a NULL handle or required pointer (all but d_frame_null, the three d_odo_* together, d_stats); d_ws not
 *   16-byte aligned; njobs, m or nobs < 0; nframes, cap, kf_list_cap, mp_list_cap, max_local, max_ref, max_mp or max_obs < 1;
 *   iters outside 1..64; nlevels outside 1..32; a mode other than the two.
 * SE2GPU_ERR_CAPACITY: nframes > 4096; njobs > 65535; nframes * cap * 3, m * 3, njobs * kf_list_cap, njobs * mp_list_cap,
 *   njobs * (max_local + max_ref) * 3, njobs * (max_mp + 1) * 3 or njobs * max_obs * 3 > 2^31 - 1; max_local + max_ref > 4096;
 *   a window size no launch width holds.
 * njobs == 0 is SE2GPU_OK and launches nothing. */
#define SE2GPU_LOCAL_BA_WS_ARRAYS 12
long long se2gpu_local_ba_ws_bytes(int njobs, int max_local, int max_ref, int max_mp, int max_obs);
int se2gpu_local_ba_ws_layout(int njobs, int max_local, int max_ref, int max_mp, int max_obs, long long* offsets,
                              long long* strides, int n);
struct se2gpu_ba_stats;
int se2gpu_local_ba_batch_device(se2gpu_matcher* h, const int32_t* d_job_kf, int njobs, const int32_t* d_win_out,
                                 const int32_t* d_local_list, const int32_t* d_ref_list, int kf_list_cap,
                                 const int32_t* d_mp_list, int mp_list_cap, int nframes, const int32_t* d_frame_id,
                                 const float* d_frame_Twb, const float* d_frame_Tcw, const uint8_t* d_frame_null,
                                 const int32_t* d_odo_to, const double* d_odo_meas, const double* d_odo_cov,
                                 const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap, const float* d_view_pos,
                                 const float* level_sigma2 /* host */, int nlevels, const float* d_pos, int m,
                                 const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr, int nobs,
                                 float fx, float cx, float cy, const double* Tbc12 /* host */, double huber_delta,
                                 double xrot_info, double z_info, int iters, int mode, int max_local, int max_ref, int max_mp,
                                 int max_obs, void* d_ws, int32_t* d_status, double* d_kf_out, double* d_mp_out,
                                 struct se2gpu_ba_stats* d_stats, int32_t* d_info);

/* Localisation on the tables where they lie in device memory: the second link of Localizer::run's per-frame chain MatchLocalMap ->
 * DoLocalBA -> UpdateCovisKFCurr -> UpdateLocalMap (src/Localizer.cpp:32-176 of the reference) for a batch of frames - the
 * observation renewal of MatchLocalMap (:220-227), the numMPCurr > 30 gate (:95-98), DoLocalBA (:233-302) with
 * addPlaneMotionSE3Expmap (src/optimizer.cpp:236-314) on the device, and KeyFrame::setPose (:298-299).  Every array pointer is
 * device memory unless marked host.  Asynchronous on the matcher's stream, ONE launch of one workgroup of 256 threads per job:
 * nothing is allocated, nothing uploaded besides kernel arguments, nothing read back, nothing waited for and no memset is issued;
 * se2gpu_matcher_sync waits for it.
 * Jobs: d_job_frame (njobs ints), the frame slot of mpKFCurr.  THE njobs SLOTS OF A BATCH MUST BE PAIRWISE DISTINCT: a job reads
 *   and writes the rows of its frame, and two jobs that share a frame would do so in no defined order.  The call cannot see the
 *   slots (they are device memory) and does not check this.
 * Frame tables (nframes slots): d_frame_Tcw (12 floats a slot: rows 0-2 of Tcw, the table of
 *   se2gpu_mappoint_parallax_batch_device), IN / OUT; d_frame_Twb (3 floats a slot: Se2 Twb), out, may be NULL.
 * Feature tables: d_kps_un (nframes x cap key points: x, y and octave are read), d_counts (nframes), cap; d_ftr_mp (nframes x cap
 *   ints, IN / OUT): KeyFrame::mDualObservations as a table, feature -> index into the point table, -1 = none; d_kf_observed
 *   (nframes x cap bytes, in / out, may be NULL): the table of se2gpu_kf_correspd_batch_device / se2gpu_match_projection_device;
 *   d_match_idx_mp (njobs x cap ints or NULL): row b is the row se2gpu_match_projection_device wrote for job b's frame.
 * Point table (m points): d_pos (m x 3 floats); d_mp_null, d_good_prl (m bytes each, may be NULL: none is null, all are good),
 *   with the meaning they have in se2gpu_covis_build_device.
 * Configuration (host): inv_level_sigma2 is a HOST array of nlevels <= 32 floats (mvInvLevelSigma2), passed as kernel arguments;
 *   fx, cx, cy (Config::Kcam; addCamPara uses fx for both axes); Tbc12 (HOST, 12 doubles: rotation row-major, translation);
 *   huber_delta (Config::TH_HUBER); xrot_info, yrot_info, z_info (PLANEMOTION_*_INFO); iters (0..64); min_obs: a job runs with more
 *   than min_obs observations - 30 for the tracked branch (:95), -1 = run always, the relocalisation branch (:133, :139).
 * Per job b with frame = d_job_frame[b], d_status[b] is the first that applies:
 *   1  the frame slot is outside 0..nframes-1.  Only d_status, the (zero) d_info words and counts, and zero d_stats are written.
 *   Renewal (:220-227), only with d_match_idx_mp: for every feature j < min(d_counts[frame], cap) with q = d_match_idx_mp[b cap + j]
 *      in 0..m-1 and point q not null (KeyFrame::addObservation returns on a null point, KeyFrame.cpp:197): d_ftr_mp[frame][j] = q
 *      and d_kf_observed[frame][j] = 1.  Any other q leaves the feature as it was.
 *   Observations = the features j < min(d_counts[frame], cap) whose d_ftr_mp lies in 0..m-1.  A value outside -1..m-1 is skipped
 *      and sets bit 0 of the job's flag word.  A point named by several features counts once and keeps the GREATEST feature index
 *      (mObservations[pMP] = idx overwrites, and both passes of the reference add in ascending feature order).  n_obs = the
 *      number of distinct points = getSizeObsMP(): null and bad-parallax points count.
 *   5  n_obs <= min_obs: not run.  d_pose_out[12 b..] is the start pose, the rows of d_frame_Tcw / d_frame_Twb are left alone,
 *      d_stats is zero.
 *   Edges (:261-288) = the observations whose point is neither null nor without good parallax, IN ASCENDING FEATURE INDEX (the
 *      reference walks a std::set of pointers; the order here is the same in every run).  Per edge xyz = the float position
 *      converted to double, uv = keyPointsUn[j].pt converted to double, w = (double)inv_level_sigma2[octave of feature j]; an
 *      octave outside 0..nlevels-1 drops the edge and sets bit 1 of the flag word.  Places come from ballots and a prefix sum.
 *   Start pose = toSE3Quat(getPose()): the 12 floats converted to double, the rotation passed through a unit quaternion as
 *      SE3Quat(R, t) does.  Prior = se2gpu_plane_motion_prior's arithmetic on that pose, on the device.
 *   0  run: optimize(iters) by the arithmetic of se2gpu_track_pose_ba.  This translation unit is compiled without floating-point
 *      contraction and that one with it: the two agree to rounding, not to the bit.
 *   6  run, and the pose came out non-finite: d_pose_out is written, the tables are not.
 *   Write-back with status 0: d_frame_Tcw[frame] = the 12 doubles of d_pose_out rounded to float (toCvMat, converter.cpp:92-107);
 *      d_frame_Twb[frame], if given, = {x, y, theta} of Tcw^-1 * Tbc^-1, computed in FP64 from d_pose_out and Tbc12, theta =
 *      atan2(R10, R00), each rounded to float once.  THE REFERENCE FORMS THIS PRODUCT WITH OpenCV's float Mat ARITHMETIC [3P]: the
 *      table value may differ from its by float rounding.  The d_frame_Twc / d_frame_P tables of the neighbouring calls stay the
 *      caller's, as they are there.
 * Outputs: d_status (njobs); d_pose_out (njobs x 12 doubles: R row-major, then t; untouched with status 1); d_stats (njobs, may be
 *   NULL: zero unless the job ran); d_info[8 b..] = {n_features, n_obs, n_edges, renewed, duplicates dropped, flag bits, 0, 0}.
 * A job's words depend on that job alone: no atomic counter, the same in every run and wherever the job stands in the batch.
 * d_ws: se2gpu_localizer_ba_ws_bytes(njobs, cap) bytes supplied by the caller, 16-byte aligned, no initialisation needed; -1 on
 *   arguments the call would refuse.  se2gpu_localizer_ba_ws_layout writes, for the SE2GPU_LOCALIZER_BA_WS_ARRAYS gathered arrays,
 *   the byte offset of job 0's slice and the stride from job to job (n >= that many; SE2GPU_ERR_INVALID otherwise or on those
 *   arguments): counts (8 ints, d_info's words), start pose (12 doubles), prior measurement (12), prior information (36, row-major,
 *   vector order (rotation, translation)), e_ftr (n_edges ints: the feature of edge i), xyz (x 3 doubles), uv (x 2), w - valid after
 *   the call for the jobs of status 0, 5 and 6.  Both helpers are host only and touch no device.
 * The argument checks come first and touch neither the handle nor a device; se2gpu_last_error names the argument:
 * SE2GPU_ERR_INVALID: a NULL handle or required pointer (all but d_frame_Twb, d_kf_observed, d_match_idx_mp, d_mp_null, d_good_prl,
 *   d_stats); d_ws not 16-byte aligned; njobs or m < 0; nframes or cap < 1; iters outside 0..64; nlevels outside 1..32;
 *   min_obs < -1.
 * SE2GPU_ERR_CAPACITY: njobs > 65535; nframes * cap, njobs * cap * 3 or m * 3 > 2^31 - 1.
 * njobs == 0 is SE2GPU_OK and launches nothing. */
#define SE2GPU_LOCALIZER_BA_WS_ARRAYS 8
long long se2gpu_localizer_ba_ws_bytes(int njobs, int cap);
int se2gpu_localizer_ba_ws_layout(int njobs, int cap, long long* offsets, long long* strides, int n);
int se2gpu_localizer_ba_batch_device(se2gpu_matcher* h, const int32_t* d_job_frame, int njobs, int nframes, float* d_frame_Tcw,
                                     float* d_frame_Twb, const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap,
                                     int32_t* d_ftr_mp, uint8_t* d_kf_observed, const int32_t* d_match_idx_mp, const float* d_pos,
                                     int m, const uint8_t* d_mp_null, const uint8_t* d_good_prl,
                                     const float* inv_level_sigma2 /* host */, int nlevels, float fx, float cx, float cy,
                                     const double* Tbc12 /* host */, double huber_delta, double xrot_info, double yrot_info,
                                     double z_info, int iters, int min_obs, void* d_ws, int32_t* d_status, double* d_pose_out,
                                     struct se2gpu_ba_stats* d_stats, int32_t* d_info);

/* ------------------------------------------------------------------------------------------
 * SE(2)-XYZ bundle adjustment  -  replaces the g2o::SparseOptimizer built by
 *   LocalMapper::localBA          /root/reference/src/LocalMapper.cpp:232-302
 *   Map::loadLocalGraph           /root/reference/src/Map.cpp:891-1053
 * through the free functions of  /root/reference/include/se2lam/optimizer.h:
 *   addCamPara (:85) addVertexSE2 (:104) addVertexSBAXYZ (:91) addEdgeSE2XYZ (:100) addEdgeSE2 (:109)
 *   estimateVertexSE2 (:107) estimateVertexSBAXYZ (:141) initOptimizer (:78)
 * and SlamOptimizer::{setForceStopFlag, initializeOptimization, optimize, clear}.
 * Vertex ids are the caller's (Map.cpp:925,966,985); poses and landmarks share one id space.
 * ------------------------------------------------------------------------------------------ */
typedef struct se2gpu_ba se2gpu_ba;

typedef struct se2gpu_ba_stats {
    int32_t iterations;   /* outer iterations executed (SparseOptimizer::optimize return value) */
    int32_t trials;       /* LM trials = linear solves */
    int32_t terminated;   /* 1 = algorithm returned Terminate (10 failed trials or rho == 0)   */
    int32_t stopped;      /* 1 = left early because *stop_flag became true */
    double chi2_init, chi2_final, lambda_final;
    double chi2_hist[64], lambda_hist[64];
    int32_t trials_hist[64];
} se2gpu_ba_stats;

int se2gpu_ba_create(se2gpu_ba** out);
void se2gpu_ba_destroy(se2gpu_ba* h);
/* Start-up pre-warm: runs one throw-away window of P key frames / L landmarks / E observations and parks its handle (code
 * objects loaded, stream + mailbox + every device buffer allocated at that size), so that the FIRST localBA of the process
 * (a SlamOptimizer constructed on the stack, LocalMapper.cpp:239) costs what the later ones do.  Off the tracking thread. */
int se2gpu_ba_reserve(int P, int L, int E);
int se2gpu_ba_clear(se2gpu_ba* h);                                   /* optimizer.clear(); clearParameters() */
int se2gpu_ba_set_stream(se2gpu_ba* h, void* hip_stream);
int se2gpu_ba_add_cam(se2gpu_ba* h, double f, double cx, double cy);  /* addCamPara: single focal length */
int se2gpu_ba_set_Tbc(se2gpu_ba* h, const double R[9], const double t[3]); /* setExtParameter(Tbc), row-major R */
int se2gpu_ba_add_vertex_se2(se2gpu_ba* h, int id, double x, double y, double theta, int fixed);
int se2gpu_ba_add_vertex_xyz(se2gpu_ba* h, int id, const double xyz[3], int marginal, int fixed);
int se2gpu_ba_add_edge_se2xyz(se2gpu_ba* h, int id_kf, int id_mp, const double uv[2], const double info[4],
                              double huber_delta);
int se2gpu_ba_add_edge_se2(se2gpu_ba* h, int id0, int id1, const double meas[3], const double info[9]);

/* Bulk form of the same calls (SoA arena filled once per key frame):
 * vertex ids: poses 0..P-1, landmarks P..P+L-1.  e_info: E x 3 (xx, xy, yy).  o_info: O x 9.
 * The four edge arrays are BORROWED: they must stay valid and unchanged until se2gpu_ba_initialize returns (which
 * validates them and copies them once, straight into the pinned upload arena); everything else is copied here. */
int se2gpu_ba_load(se2gpu_ba* h, int P, int L, int E, int O,
                   const double* poses, const uint8_t* fixed, const double* lms,
                   const int32_t* e_kf, const int32_t* e_lm, const double* e_uv, const double* e_info,
                   const int32_t* o_i, const int32_t* o_j, const double* o_meas, const double* o_info,
                   double huber_delta);

/* ---- SE3-expmap graphs: the marginalising local bundle adjustment of
 *   Map::loadLocalGraph(optimizer, vpEdgesAll, vnAllIdx)   /root/reference/src/Map.cpp:414-566
 *   LocalMapper::removeOutlierChi2                          /root/reference/src/LocalMapper.cpp:172-230
 * on the same handle type: a graph is EITHER SE(2) (add_vertex_se2 ...) OR SE3 (the calls below), decided by its first
 * pose vertex.  pose12 = rotation row-major (9) then translation (3) of Tcw (x_c = R x_w + t); 6x6 information matrices
 * row-major in g2o's vector order (rotation, translation).  Replaces, of /root/reference/include/se2lam/optimizer.h:
 *   addVertexSE3Expmap (:88)                     -> se2gpu_ba_add_vertex_se3
 *   addPlaneMotionSE3Expmap (:82)                -> se2gpu_plane_motion_prior (host) + se2gpu_ba_add_prior_se3
 *   addEdgeSE3Expmap (:94)                       -> se2gpu_ba_add_edge_se3   (error = log(T_id1^-1 * measure * T_id0))
 *   addEdgeXYZ2UV (:97)                          -> se2gpu_ba_add_edge_xyz2uv (information = inv_sigma2 * I, Huber)
 *   addVertexSBAXYZ / estimateVertexSBAXYZ       -> se2gpu_ba_add_vertex_xyz / se2gpu_ba_get_xyz (shared)
 *   estimateVertexSE3Expmap (:138)               -> se2gpu_ba_get_se3
 *   EdgeProjectXYZ2UV::computeError() + chi2()   -> se2gpu_ba_edge_chi2 (all edges, in the order they were added)
 * initialize / optimize / optimize_batch / chi2 / clear are the common ones.  Single GPU only. */
int se2gpu_ba_add_vertex_se3(se2gpu_ba* h, int id, const double pose12[12], int fixed);
/* ---- pose graphs: GlobalMapper::GlobalBA (/root/reference/src/GlobalMapper.cpp:328-535).
 * A graph whose first pose vertex is added with se2gpu_ba_add_vertex_iso3 is a g2o::VertexSE3 pose graph (poses T_w_c,
 * update estimate * fromVectorMQT(d)); se2gpu_ba_add_prior_se3 then adds an EdgeSE3Prior (what
 * addVertexSE3PlaneMotion, optimizer.h:123, attaches: build it with se2gpu_plane_motion_prior_iso3), se2gpu_ba_add_edge_se3
 * an EdgeSE3 (addEdgeSE3, optimizer.h:129: error toVectorMQT(measure^-1 * T_id0^-1 * T_id1); several edges between the
 * same two key frames are allowed - odometry + feature edge).  Vector order (translation, rotation) for errors and
 * information matrices.  se2gpu_ba_get_se3 = estimateVertexSE3 (:135), se2gpu_ba_edge_chi2 = EdgeSE3::chi2() of every
 * edge in insertion order (the feature-edge rejection of GlobalMapper.cpp:415-437, 455-476).  No landmarks. */
int se2gpu_ba_add_vertex_iso3(se2gpu_ba* h, int id, const double Twc12[12], int fixed);
int se2gpu_plane_motion_prior_iso3(const double* Twc12, const double* Tbc12, double xrot_info, double yrot_info,
                                   double z_info, double* meas12, double* info36);
int se2gpu_ba_add_prior_se3(se2gpu_ba* h, int id, const double meas12[12], const double info36[36]);
int se2gpu_ba_add_edge_se3(se2gpu_ba* h, int id0, int id1, const double meas12[12], const double info36[36]);
int se2gpu_ba_add_edge_xyz2uv(se2gpu_ba* h, int id_mp, int id_kf, const double uv[2], double inv_sigma2, double huber_delta);
int se2gpu_ba_get_se3(se2gpu_ba* h, int id, double pose12[12]);
int se2gpu_ba_edge_chi2(se2gpu_ba* h, double* chi2, int cap);

/* Sparsifier::DoMarginalizeSE3XYZ (/root/reference/src/sparsifier.cpp:105-275) for a batch of key-frame pairs - SURVEY.md
 * section 8f.4: the feature constraint (relative pose + 6x6 information, order (translation, rotation) of
 * SE3Quat::toMinimalVector) that GlobalMapper::CreateFeatEdge (src/GlobalMapper.cpp:744-840) stores in mFtrMeasureFrom and
 * GlobalBA turns into an EdgeSE3.  Pair p: kf12[p] = T_w_c of the two key frames (2 x 12), its map points
 * mp_xyz[mp_ptr[p] .. mp_ptr[p+1]) and its measurements [m_ptr[p], m_ptr[p+1]): m_kf in {0, 1} (others are ignored, as
 * :117-119), m_mp = index of the point inside the pair, m_info = 3x3 information (row-major; MeasSE3XYZ::info).
 * z_out12[p] = pose12 of KF0^-1 * KF1, info_out36[p] row-major.  One wave per pair; host buffers. */
int se2gpu_sparsify_se3xyz(int npairs, const double* kf12, const int32_t* mp_ptr, const double* mp_xyz,
                           const int32_t* m_ptr, const int32_t* m_kf, const int32_t* m_mp, const double* m_info,
                           double* z_out12, double* info_out36);

/* GlobalMapper::CreateFeatEdge (/root/reference/src/GlobalMapper.cpp:737-843) for a batch of key-frame pairs: the bundle
 * adjustment of the two key frames and their common map points - OptKFPair (:847-927: key frame 0 fixed, 15 iterations) or
 * OptKFPairMatch (:929-1032: both free, 30 iterations, then every point with an edge chi2 above 5.0 is dropped) - followed on
 * the device by Sparsifier::DoMarginalizeSE3XYZ on the optimised poses and the surviving points.  The graph is g2o's
 * VertexSE3 (T_w_c) with the EdgeSE3Prior of addVertexSE3PlaneMotion (built here from the INPUT pose, Tbc and the three
 * informations, as se2gpu_plane_motion_prior_iso3 does), marginalised VertexPointXYZ, and one EdgeSE3PointXYZ per point and
 * key frame (offset = identity, Huber huber_delta), Levenberg-Marquardt.  One wave per pair; host buffers.
 * Pair p: kf12[p] (2 x 12), its points mp_xyz[mp_ptr[p] .. mp_ptr[p+1]) (start values), per point m_z (2 x 3: the point in
 * key frame 0's camera, then in key frame 1's: KeyFrame::mViewMPs) and m_info (2 x 9, row-major: mViewMPsInfo).
 * Outputs: kf12_out (optimised T_w_c), mp_xyz_out, outlier (per point; always 0 in COVIS mode or with outlier_chi2 <= 0),
 * edge_chi2 (per point x 2, not robustified), stats (per pair, may be NULL), z_out12 / info_out36 as
 * se2gpu_sparsify_se3xyz, and info4 per pair = {status, points, outliers, points handed to the sparsifier}:
 *   status 0  constraint written
 *   status 1  fewer than min_points points (counted before the rejection, as :790 does): nothing is run, kf12_out and
 *             mp_xyz_out are the input, z_out12 / info_out36 / stats zero
 *   status 2  a non-finite result: z_out12 / info_out36 zero
 * SE2GPU_ERR_INVALID: a NULL required pointer, a mode other than the two, mp_ptr not starting at 0 or decreasing, iters
 * outside 1..64 (the histories of se2gpu_ba_stats).  SE2GPU_ERR_CAPACITY: npairs >= 65536.  All before any device use. */
#define SE2GPU_FEAT_EDGE_COVIS 0   /* OptKFPair:      KF0 fixed, no rejection; reference: 15 iterations, >= 10 points */
#define SE2GPU_FEAT_EDGE_MATCH 1   /* OptKFPairMatch: both free, chi2 rejection; reference: 30 iterations, >= 3 matches */
int se2gpu_feat_edge_batch(int npairs, int mode, int iters, int min_points,
        const double* kf12,            /* npairs x 2 x 12, T_w_c */
        const double* Tbc12, double xrot_info, double yrot_info, double z_info,
        const int32_t* mp_ptr, const double* mp_xyz,          /* CSR over pairs; start values of the points */
        const double* m_z, const double* m_info,              /* per point: 2 x 3 and 2 x 9 (KF0 then KF1) */
        double huber_delta, double outlier_chi2,
        double* kf12_out, double* mp_xyz_out, uint8_t* outlier, double* edge_chi2 /* per point x 2 */,
        int32_t* info4 /* per pair: status, points, outliers, points handed to the sparsifier */,
        se2gpu_ba_stats* stats /* per pair, may be NULL */,
        double* z_out12, double* info_out36);

/* CreateFeatEdge on the tables where they lie in device memory: se2gpu_feat_edge_batch behind a gather kernel, for the pairs of
 * se2gpu_covis_pairs_device (its d_common) or of se2gpu_track_loop_verify_batch_device (its d_matches_mp).  Every array pointer
 * is device memory.  Asynchronous on the matcher's stream (five launches, one memset with d_stats): nothing is allocated,
 * nothing uploaded besides kernel arguments, nothing read back and nothing waited for; se2gpu_matcher_sync waits for it.
 * mode, iters, min_points, huber_delta, outlier_chi2, xrot_info, yrot_info, z_info as for se2gpu_feat_edge_batch; Tbc12 is a
 * HOST pointer to 12 doubles, copied into a kernel argument.
 * Common inputs: d_pair_a / d_pair_b (npairs frame slots: _pKFFrom, _pKFTo); d_frame_Twc (nframes x 12 floats, rows 0-2 of
 * cvu::inv(Tcw): the table of se2gpu_mappoint_parallax_batch_device; the rows of the 3 x 4 matrix become rotation (9) and
 * translation (3) of kf12, float -> double exactly, as toIsometry3D does); d_pos (m x 3 floats, MapPoint::getPos(), the array the
 * parallax call writes); row_cap = the point slots a pair gets in every per-point array: pair p's rows start at p * row_cap.
 * SE2GPU_FEAT_EDGE_COVIS (GlobalMapper.cpp:741-750, :847-927): d_pair_out (4 ints per pair) and d_common (3 ints per entry,
 *   list_cap entries per pair) as se2gpu_covis_pairs_device wrote them for the same pair arrays; d_obs_view (nobs x 3 floats),
 *   d_obs_info (nobs x 9).  Pair p takes the entries i < min(n_same, list_cap, row_cap) in list order (ascending point index,
 *   the stand-in for the reference's std::set order).  An entry {point, e_a, e_b} is valid when point lies in 0..m-1 and e_a,
 *   e_b in 0..nobs-1; invalid entries are dropped and the rest compacted in order at the head of the row.  A point's start
 *   value is d_pos[point], its m_z = d_obs_view[e_a], d_obs_view[e_b], its m_info = d_obs_info[e_a], d_obs_info[e_b].
 *   raw = n_same.  A pair with n_same < 0 or a slot outside 0..nframes-1 is a pair of no points.
 *   The match route's arrays are not read and may be NULL.
 * SE2GPU_FEAT_EDGE_MATCH (:929-1032): d_matches (npairs x cap ints) with d_counts (nframes) and cap in the layout of the verify
 *   call's d_matches_mp; d_ftr_mp (nframes x cap ints: the map point KeyFrame::getObservation(idx) names, as an index into the
 *   point table, or -1); d_view_pos (nframes x cap x 3 floats, mViewMPs, the table of se2gpu_kf_correspd_batch_device) and
 *   d_view_info (nframes x cap x 9, mViewMPsInfo).  Raw matches by the verify call's rule: i < min(counts[a], cap) with a
 *   value j in 0..min(counts[b], cap)-1, in ascending i (std::map<int,int>); raw = their number (:790 tests it).  A raw match
 *   becomes a point when d_ftr_mp[a][i] lies in 0..m-1 and d_ftr_mp[b][j] >= 0 (:960-965): start value d_pos[d_ftr_mp[a][i]]
 *   (:968), m_z / m_info from (a, i) and (b, j) of the two view tables (:971-976).  Points beyond row_cap are cut.  A pair with
 *   a slot outside 0..nframes-1 has no matches.  The reference indexes vIdMPin1 by the match counter and the points by the
 *   kept-point counter (:956-962 against :1000), so after a skipped match it rejects the wrong points; THE LIBRARY DOES NOT
 *   REPRODUCE THAT: the outlier flag of a point is the flag of that point.
 *   The covisibility route's arrays are not read and may be NULL.
 * A slot out of range gives the identity as that key frame's pose.
 * Outputs: d_kf12_out (npairs x 24 doubles), d_z_out12 (npairs x 12), d_info_out36 (npairs x 36) as the host call's; optional
 * (NULL: not wanted) d_mp_xyz_out (npairs x row_cap x 3 doubles), d_outlier (npairs x row_cap bytes), d_edge_chi2 (npairs x
 * row_cap x 2), whose rows are left untouched from `points` on, and d_stats (per pair);
 * d_info8[8p..] = {status, points, outliers, points handed to the sparsifier, raw, dropped, cut, 0}: points = the gathered
 * count; dropped = invalid entries, or raw matches without both points; cut = 1 when list_cap or row_cap truncated the pair.
 *   status 1  raw < min_points: nothing is run, kf12_out is the input pose, the constraint is zero (outlier / edge_chi2 of
 *             the gathered points are 0, mp_xyz_out their start values)
 *   otherwise the pair is optimised on its gathered points, exactly as se2gpu_feat_edge_batch does with those rows and a
 *             min_points that lets them through - a pair whose gather came out empty included
 *   status 2  a non-finite result or constraint: the constraint is zero
 * A pair's words depend on that pair alone: no atomics, the same in every run and wherever the pair stands in the batch.
 * d_ws: se2gpu_feat_edge_ws_bytes(npairs, row_cap) bytes supplied by the caller, 8-byte aligned, no initialisation needed (the
 * call fills every word it reads).  se2gpu_feat_edge_ws_bytes returns -1 on arguments the call would refuse (npairs < 0 or
 * >= 65536, row_cap < 1, 2 * npairs * row_cap > 2^31 - 1).  se2gpu_feat_edge_ws_layout writes the byte offsets inside d_ws
 * of the SE2GPU_FEAT_EDGE_WS_ARRAYS gathered arrays (n >= that many; SE2GPU_ERR_INVALID otherwise or on those arguments):
 * counts (npairs ints, followed by raw, dropped and cut, npairs ints each), kf12 (npairs x 24 doubles), prior measurement
 * (npairs x 24), prior information (npairs x 72), start xyz (npairs x row_cap x 3 doubles), m_z (x 6), m_info (x 18) - valid
 * after the call.  Both helpers are host only and touch no device.
 * The argument checks come first and touch neither the handle nor a device:
 * SE2GPU_ERR_INVALID: a NULL handle, Tbc12, common array, d_ws, d_info8, d_kf12_out, d_z_out12, d_info_out36 or array of the
 *   mode's route; a mode other than the two; iters outside 1..64; npairs, m or nobs < 0; nframes, cap, row_cap or list_cap
 *   < 1 (the scalars of both routes are checked whatever the mode: a caller of one route passes 0 / 1 / 1 for the other's).
 * SE2GPU_ERR_CAPACITY: npairs >= 65536; 2 * npairs * row_cap > 2^31 - 1; nframes * cap > 2^31 - 1.
 * npairs == 0 is SE2GPU_OK and launches nothing. */
#define SE2GPU_FEAT_EDGE_WS_ARRAYS 7
long long se2gpu_feat_edge_ws_bytes(int npairs, int row_cap);
int se2gpu_feat_edge_ws_layout(int npairs, int row_cap, long long* offsets, int n);
int se2gpu_feat_edge_batch_device(se2gpu_matcher* h, int mode, int iters, int min_points, double huber_delta, double outlier_chi2,
        const double* Tbc12 /* host */, double xrot_info, double yrot_info, double z_info,
        const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs, int nframes,
        const float* d_frame_Twc, const float* d_pos, int m, int row_cap,
        const int32_t* d_pair_out, const int32_t* d_common, int list_cap,           /* covisibility route */
        const float* d_obs_view, const float* d_obs_info, int nobs,
        const int32_t* d_matches, const int32_t* d_counts, int cap,                  /* match route */
        const int32_t* d_ftr_mp, const float* d_view_pos, const float* d_view_info,
        void* d_ws, int32_t* d_info8, double* d_kf12_out, double* d_z_out12, double* d_info_out36,
        double* d_mp_xyz_out, uint8_t* d_outlier, double* d_edge_chi2, se2gpu_ba_stats* d_stats);

/* Map::loadLocalGraph(SlamOptimizer&) (/root/reference/src/Map.cpp:891-1022) as ONE call on a POD view of the local
 * window - SURVEY.md section 8f.1.  The caller flattens its pointer graph once per key frame (INTEGRATION.md shows the
 * 30 lines that do it with one hash map instead of the reference's std::find per observation); the library applies
 * the reference's vertex numbering (local key frame i -> id i, reference key frame i -> n_local + i, map point i ->
 * n_local + n_ref + 1 + i), its fixed rule (no reference key frames: the local one with the smallest KeyFrame::id is
 * fixed; KeyFrame::id == 1 always; reference key frames always), inverts the PreSE2 covariances, and evaluates the
 * per-observation information matrices (:1024-1049) on the device during se2gpu_ba_initialize.  The optimizer must be
 * empty; afterwards initialize / optimize / get_* as usual with those ids. */
typedef struct se2gpu_local_graph {
    int32_t n_local_kf, n_ref_kf, n_mp, n_obs;
    /* key frames: mLocalGraphKFs first, then mRefKFs                                    [n_local_kf + n_ref_kf] entries */
    const int32_t* kf_id;     /* KeyFrame::id */
    const float* kf_Twb;      /* Se2 Twb: x, y, theta                                      x 3 */
    const float* kf_Rcw;      /* rotation block of KeyFrame::Tcw (CV_32F), row-major       x 9 */
    /* odometry of the local key frames (KeyFrame::preOdomFromSelf)                       [n_local_kf] entries, may be NULL */
    const int32_t* odo_to;    /* position of preOdomFromSelf.first in mLocalGraphKFs, -1 = not in the window / null */
    const double* odo_meas;   /* PreSE2::meas                                              x 3 */
    const double* odo_cov;    /* PreSE2::cov, row-major                                    x 9 */
    /* map points (mLocalGraphMPs) and their observations, grouped by map point            [n_mp] / [n_obs] entries */
    const float* mp_pos;      /* MapPoint::getPos()                                        x 3 */
    const int32_t* obs_mp;    /* map point of the observation, nondecreasing */
    const int32_t* obs_kf;    /* observing key frame: position in the list above, -1 = in neither list (skipped, :1016) */
    const float* obs_uv;      /* keyPointsUn[ftrIdx].pt                                    x 2 */
    const float* obs_lc;      /* mViewMPs[ftrIdx]                                          x 3 */
    const float* obs_sigma2;  /* mvLevelSigma2[octave] */
    float fx, cx, cy;         /* Config::Kcam (addCamPara uses fx for both axes) */
    double Rbc[9], tbc[3];    /* Config::bTc, rotation row-major */
    float huber_delta;        /* Config::TH_HUBER */
    float xrot_info, z_info;  /* Config::PLANEMOTION_XROT_INFO, PLANEMOTION_Z_INFO */
} se2gpu_local_graph;
int se2gpu_ba_load_local_graph(se2gpu_ba* h, const se2gpu_local_graph* graph);

/* Map::updateLocalGraph() (/root/reference/src/Map.cpp:285-331) on a CSR view of the map - SURVEY.md section 8 row a25: the
 * local window of the current key frame = key frames within `search_level` (3 in the reference) covisibility hops, the
 * map points they observe, and as reference key frames every other observer of those points.  Pure host code (no device
 * needed); the three outputs are positions in the view's arrays, ordered by KeyFrame::id / MapPoint::id like the
 * reference's sets, i.e. exactly mLocalGraphKFs, mRefKFs, mLocalGraphMPs - the lists se2gpu_ba_load_local_graph takes.
 * Output arrays may be NULL (sizes only); capacities n_kf / n_kf / n_mp always suffice. */
typedef struct se2gpu_map_view {
    int32_t n_kf, n_mp;
    const int32_t* kf_id;                        /* KeyFrame::id                                  [n_kf] */
    const int32_t* covis_ptr; const int32_t* covis_idx;   /* KeyFrame::getAllCovisibleKFs() as CSR        [n_kf + 1] */
    const int32_t* kf_mp_ptr; const int32_t* kf_mp_idx;   /* KeyFrame::getAllObsMPs(false) as CSR         [n_kf + 1] */
    const int32_t* mp_id;                        /* MapPoint::id                                  [n_mp] */
    const int32_t* mp_kf_ptr; const int32_t* mp_kf_idx;   /* MapPoint::getObservations() as CSR           [n_mp + 1] */
} se2gpu_map_view;
int se2gpu_map_update_local_graph(const se2gpu_map_view* map, int current_kf, int search_level, int32_t* local_kfs,
                                  int* n_local, int32_t* ref_kfs, int* n_ref, int32_t* local_mps, int* n_mps);

/* initializeOptimization(0): freezes the graph, builds the device-side SoA + reduction plans (on the device).
 * A second call on an initialised handle is g2o's "initialise again over the edges of level 0": supported for the pose graph
 * (VertexSE3 / EdgeSE3, the graph of GlobalMapper::GlobalBA, /root/reference/src/GlobalMapper.cpp:421-483): the vertices keep
 * their current estimates, edges moved to another level by se2gpu_ba_set_edge_level are left out.  For the landmark models
 * it returns SE2GPU_ERR_STATE. */
int se2gpu_ba_initialize(se2gpu_ba* h);
/* g2o::OptimizableGraph::Edge::setLevel(level) of the `edge`-th EdgeSE3 added to a pose graph (the index
 * se2gpu_ba_edge_chi2 reports it under); takes effect at the next se2gpu_ba_initialize. */
int se2gpu_ba_set_edge_level(se2gpu_ba* h, int edge, int level);
/* restores every vertex estimate to the value the device graph was built with (device-to-device): the value it was added with -
 * or, on a pose graph that was initialised a second time, the estimates that second se2gpu_ba_initialize started from (g2o has
 * no such reset; a re-initialise moves the reset point) */
int se2gpu_ba_reset_estimates(se2gpu_ba* h);
/* ... of `count` windows with one launch (the companion of se2gpu_ba_optimize_batch for a mapper that re-optimises the same
 * windows): ordered before any later operation on each of the windows */
int se2gpu_ba_reset_estimates_batch(se2gpu_ba** handles, int count);

#define SE2GPU_BA_LM 0  /* OptimizationAlgorithmLevenberg, g2o policy (optimizer.h:32) */
#define SE2GPU_BA_GN 1  /* plain Gauss-Newton: lambda = 0, every step accepted           */
/* optimize(iters); stop_flag mirrors setForceStopFlag(bool*) (LocalMapper.cpp:246), may be NULL. */
int se2gpu_ba_optimize(se2gpu_ba* h, int iters, int mode, const volatile uint8_t* stop_flag, int verbose,
                       se2gpu_ba_stats* stats);
/* optimize(iters) of `count` independent windows at once - one initialised handle per window, each on its own stream.
 * The Levenberg-Marquardt controller of every window runs on the device, so all windows are enqueued before the first
 * wait and the GPU works on them concurrently (a 50-KF local window occupies a few per cent of an MI355X).  This is the
 * throughput form for a mapper that keeps several local windows (or several robots' maps) in flight; results are those
 * of calling se2gpu_ba_optimize on every handle in turn - bit for bit on paths 0 and 1, equal to rounding on the resident
 * path 2 (see se2gpu_ba_last_batch_path).  A batch may mix SE(2) and SE3-expmap windows.  stats: NULL or `count` entries. */
int se2gpu_ba_optimize_batch(se2gpu_ba** handles, int count, int iters, int mode, const volatile uint8_t* stop_flag,
                             se2gpu_ba_stats* stats);
/* Which of its three paths the calling thread's last se2gpu_ba_optimize_batch took (-1: none yet): 0 = one stream per window,
 * 1 = lock step (one launch per stage for all windows; SE(2) windows only), 2 = resident (one workgroup per window for its
 * whole optimize(): batches of SE2GPU_BA_RESIDENT_MIN = 96 windows or more whose windows fit a compute unit's LDS - SE(2) windows
 * (csrc/ba_window.hip, up to ~60 free key frames) and SE3-expmap windows (csrc/ba_window3.hip, up to 27 free key frames at 256
 * threads, 29 at 128), in one batch if need be; pose graphs never; its sums are atomic, so its results equal the other paths' to
 * rounding, not to the bit).  SE2GPU_BA_RESIDENT=0 / 1 forces the choice.
 * Odometry shapes: a window with a PreEdgeSE2 self loop (i, i) keeps the batch off the resident path, even when it is forced;
 * a self loop or a pair of key frames joined by two PreEdgeSE2 (in either direction) keeps it off the lock-step path (such a
 * window runs in synchronous mode).  Edges in any order and direction, and any number of them at one key frame, are taken. */
int se2gpu_ba_last_batch_path(void);
int se2gpu_ba_get_se2(se2gpu_ba* h, int id, double xyt[3]);   /* estimateVertexSE2   */
int se2gpu_ba_get_xyz(se2gpu_ba* h, int id, double xyz[3]);   /* estimateVertexSBAXYZ */
int se2gpu_ba_get_all(se2gpu_ba* h, double* poses /*P*3, in pose-add order*/, double* lms /*L*3*/);
double se2gpu_ba_chi2(se2gpu_ba* h);                          /* activeRobustChi2() at the current estimate; <0 on error */

/* Parity introspection: reduced (Schur) system at the current estimate and damping `lambda`:
 * S (3P x 3P row-major, fixed poses -> identity rows), bs (3P).  P counts poses in add order. */
int se2gpu_ba_debug_reduced_system(se2gpu_ba* h, double lambda, double* S, double* bs);
/* ... and its dense solve on the device (the LL^T that stands in for CHOLMOD): x (3P) with S x = bs;
 * *factor_ok = 0 when a pivot was not positive. */
int se2gpu_ba_debug_solve(se2gpu_ba* h, double lambda, double* x, int* factor_ok);
/* Which dense solver an initialised handle runs: 0 = the dataflow launch (k_chol_tiles), 1 = one launch per block column
 * by configuration (SE2GPU_BA_CHOL=steps, more than 64 tile rows), 2 = one launch per block column because a dataflow
 * dependency timed out earlier in the handle's life (reported once on stderr), 3 = host solve (SE2GPU_BA_HOST_SOLVE=1).
 * Tests use it to make sure that results were not produced by the fallback. */
int se2gpu_ba_debug_solver_path(const se2gpu_ba* h);
/* The speculating trial slot of the single-window SE(2) run (k_update<true> also linearises the trial state; SE2GPU_BA_SPECULATE=0
 * switches it off), for the handle's last optimize(): *runs = trial slots whose stand-alone linearisation did its work (the
 * first trial, every retry, every accept whose new damping was not lambda / 3), *skips = slots where it returned at once because
 * the slot before had already written the records; runs + skips = trials.  *twin_bytes = size of the handle's second record set
 * (0 until a run of the handle has speculated).  Any of the three pointers may be NULL. */
int se2gpu_ba_debug_linearize_counts(const se2gpu_ba* h, int* runs, int* skips, long long* twin_bytes);
/* Test introspection: idle sets in the library's two process-wide lease pools - {plan caches of the lock-step batch driver,
 * staging buffers of se2gpu_ba_reset_estimates_batch}.  A set is leased per call and returned, whichever thread calls. */
int se2gpu_ba_debug_pool_sizes(int out2[2]);
/* Soak-test introspection of the dataflow solve's tile hand-offs.  With SE2GPU_BA_CHOL_VERIFY=1 in the environment every
 * published half-slab carries a checksum and every consumer checks its loads against it: counts2 = {mismatches, half-slabs
 * checked}; records (cap x 8 words, may be NULL): {epoch, consumer task, kind << 32 | tile row << 16 | column, slab << 8 |
 * part, consumer XCC, got, want, 100 MHz time stamp}.  SE2GPU_ERR_STATE when the handle does not run in that mode. */
int se2gpu_ba_debug_chol_verify(se2gpu_ba* h, unsigned long long* counts2, unsigned long long* records, int cap);
/* The plan of the dense pose solve (tile tasks, their dependency lists, the fill-reducing order of the poses) for a P x P
 * block pattern, computed on the host without a device - what stands in for CHOLMOD's symbolic analysis behind
 * /root/reference/include/se2lam/optimizer.h:31.  Test introspection (tests/test_solve_plan.py). */
int se2gpu_ba_debug_solve_plan(int P, int D, const uint8_t* pattern, int allow_nd, int* nsys, int* nbc, int* depth, int* ntask,
                               int* ndep, int32_t* pose_off, int32_t* tasks4, int task_cap, int32_t* deps, int dep_cap);
/* the same with the tile size of the dense solve as an argument (32 or 64) */
int se2gpu_ba_debug_solve_plan_tile(int P, int D, const uint8_t* pattern, int allow_nd, int tile, int* nsys, int* nbc, int* depth, int* ntask,
                                    int* ndep, int32_t* pose_off, int32_t* tasks4, int task_cap, int32_t* deps, int dep_cap);
/* A tile task's list is in the order in which its block columns are published (by depth on the dependency chain, ties by
 * index), and the task polls the last `neager` entries - the columns of the largest depth - in earnest: one int per task of
 * the plan above, in task order (1 for the x tasks, 0 for a task with an empty list). */
int se2gpu_ba_debug_solve_plan_neager(int P, int D, const uint8_t* pattern, int allow_nd, int tile, int32_t* neager, int cap);
/* ... and of the plan an initialised handle runs, read back from the device: *nsys = order of the (padded) system,
 * *permuted = 1 when the fill-reducing order was taken, *ntask = tasks; neager (cap >= *ntask ints) may be NULL. */
int se2gpu_ba_debug_plan_neager(se2gpu_ba* h, int* nsys, int* permuted, int* ntask, int32_t* neager, int cap);
/* The flat plan records of the SE(2) model's k_reduce2 (one per group slot, 11 x 4 ints: the group descriptor, {column of a,
 * column of b, blk_odo, both poses free}, {o_i, o_j, 0, 0} of the block's PreEdgeSE2 edge, then lane t's pair indices
 * {i_t, j_t, i_(8+t), j_(8+t)}, t < 8, clamped to the chunk's last pair).  The first form runs the record builder on host
 * arrays, without a device; pair_i / pair_j / pose_off / o_i / o_j may be NULL where no descriptor refers to them. */
int se2gpu_ba_debug_flat_records_host(int nslots, const int32_t* grp4, const int32_t* blk_a, const int32_t* blk_b, const int32_t* blk_odo,
                                      const int32_t* pair_i, const int32_t* pair_j, const uint8_t* fixed, const int32_t* pose_off,
                                      const int32_t* o_i, const int32_t* o_j, int32_t* flat);
/* ... the second reads back what an initialised handle uses, with its group descriptors (cap_slots * 4 and cap_slots * 44
 * ints; NULL for both returns *nslots alone; *nslots = 0: the handle runs without the records, SE2GPU_BA_REDUCE_FLAT=0). */
int se2gpu_ba_debug_flat_records(se2gpu_ba* h, int32_t* grp4, int32_t* flat, int cap_slots, int* nslots);
/* The off-diagonal workgroups of the SE(2) model's k_reduce2: out = {workgroups of the plan, those that hold a group of a block
 * with a contributor pair or a PreEdgeSE2 edge (the plan packs the empty blocks behind all others; equal to the first without
 * that order: SE2GPU_BA_REDUCE_EMPTY=0, sharded handles, the 6-DoF models), those the next reduction launches}. */
int se2gpu_ba_debug_reduce_grid(const se2gpu_ba* h, int out[3]);
/* The host builder's packing of a graph (edges sorted by landmark) into group descriptors, without a device: grp4 (cap_slots * 4
 * ints, or NULL) and out = {group slots, workgroups, workgroups of the non-empty blocks}.  empty_last: the order above;
 * odo_ok = 0: the PreEdgeSE2 edges stay out of the block plan (self loops, duplicates) and only mark their blocks non-empty. */
int se2gpu_ba_debug_plan_host(int P, int L, int E, const int32_t* e_kf, const int32_t* e_lm, const uint8_t* fixed, int O,
                              const int32_t* o_i, const int32_t* o_j, int odo_ok, int empty_last, int32_t* grp4, int cap_slots,
                              int out[3]);
/* Test introspection of the SE(3) arithmetic the 6-DoF kernels share (csrc/se3_math.h): runs function `op` on the device, one
 * item per thread, in one launch.  Every item has 24 doubles of input and 36 of output, whatever the op (unused ones are read
 * as given and written as zero); a pose is pose12 = R row-major (9), t (3):
 *   EXP (omega, upsilon) -> pose          LOG pose -> (omega, upsilon)         MUL pose A, pose B -> se3_mul(A, B)
 *   NORMALIZE R (9) -> R (9)              QUAT_OF R (9) -> (w, x, y, z)        TO_MQT pose -> 6      FROM_MQT 6 -> pose
 *   ADJ pose -> 6x6                       JAC_RIGHT pose E -> 6x6              JAC_LEFT_INV pose A, pose B -> 6x6
 *   LOG_EXP (omega, upsilon) -> se3_log(se3_exp(.)) */
enum {
    SE2GPU_SE3_EXP = 0, SE2GPU_SE3_LOG, SE2GPU_SE3_MUL, SE2GPU_SE3_NORMALIZE, SE2GPU_SE3_QUAT_OF, SE2GPU_SE3_TO_MQT,
    SE2GPU_SE3_FROM_MQT, SE2GPU_SE3_ADJ, SE2GPU_SE3_JAC_RIGHT, SE2GPU_SE3_JAC_LEFT_INV, SE2GPU_SE3_LOG_EXP, SE2GPU_SE3_OPS
};
int se2gpu_debug_se3(int op, int n, const double* in /* n x 24 */, double* out /* n x 36 */);
/* Test introspection of the integer wave and workgroup primitives the batch kernels share (csrc/wave_int.h): one workgroup of
 * `block` threads (64, 256 or 1024) walks in[0..n) in chunks of `block` and applies `op` to every chunk; lanes past n contribute the
 * identity (0; INT_MAX for MIN, INT_MIN for MAX).  A wave is 64 consecutive values; the I32 ops take (int)in[i].
 *   SUM / MIN / MAX        out[i] = the sum / minimum / maximum over i's wave, as int
 *   SCAN_I32 / SCAN_I64    out[i] = the inclusive prefix sum inside i's wave
 *   RANK                   out[i] = the number of j < i in i's wave with in[j] != 0
 *   BLOCK_SCAN_I32 / _I64  out[i] = in[0] + .. + in[i - 1]: the workgroup's exclusive scan of every chunk on top of the total of the
 *                          chunks before it, all on the same words of LDS; out[n] = the sum of all (out has n + 1 words)
 *   FRESH_SCAN_I32 / _I64  the same with the barrier in front of the LDS write dropped; one chunk, n <= block */
enum {
    SE2GPU_WI_SUM = 0, SE2GPU_WI_MIN, SE2GPU_WI_MAX, SE2GPU_WI_SCAN_I32, SE2GPU_WI_SCAN_I64, SE2GPU_WI_RANK, SE2GPU_WI_BLOCK_SCAN_I32,
    SE2GPU_WI_BLOCK_SCAN_I64, SE2GPU_WI_FRESH_SCAN_I32, SE2GPU_WI_FRESH_SCAN_I64, SE2GPU_WI_OPS
};
int se2gpu_debug_wave_int(int op, int block, int n, const long long* in, long long* out);

/* Track::doTriangulate (/root/reference/src/Track.cpp:378-419) for every match of a frame pair in one device pass -
 * SURVEY section 8(f).3.  Per feature i of the reference key frame with match_idx[i] >= 0 and no map point yet:
 *   pos = cvu::triangulate(kps_ref[i].pt, kps_cur[match_idx[i]].pt, P_ref, P_cur)   (cvutil.cpp:46-59: DLT, smallest
 *         right singular vector of the 4x4 system; one-sided Jacobi like cv::SVD, FP64 inside, FP32 in / out)
 *   Config::acceptDepth(pos.z) (Config.cpp:188-190)  ? pos_out[i] = pos, good_parallax[i] = cvu::checkParallax(0, Ocam,
 *         pos, min_degree) (cvutil.cpp:92-98)        : match_idx[i] = -1
 * Features with has_observation[i] != 0 are only counted (*n_tracked_old; the caller keeps the key frame's map point).
 * P_ref = Config::PrjMtrxEye, P_cur = Config::Kcam * Tcr.rowRange(0,3): 3x4 row-major float.  Host buffers. */
int se2gpu_triangulate(int n, const se2gpu_keypoint* kps_ref, const se2gpu_keypoint* kps_cur, int n_cur,
                       int32_t* match_idx, const uint8_t* has_observation, const float* P_ref, const float* P_cur,
                       const float* Ocam, float lower_depth, float upper_depth, int min_degree, float* pos_out,
                       uint8_t* good_parallax, int* n_good, int* n_tracked_old);

/* Track::removeOutliers (/root/reference/src/Track.cpp:308-344) - SURVEY section 8(f).3: the epipolar filter applied to
 * the MatchByWindow result in Track::mTrack (Track.cpp:134).  The handle owns a stream and the staging / device buffers
 * of the calling thread (Track is single-threaded); it is not thread-safe.
 *   se2gpu_track_fundamental_mask  = cv::findFundamentalMat(pt1, pt2, mask) with the defaults FM_RANSAC, 3 px, 0.99
 *       [OpenCV 3.2]: n < 7 no mask (all 0 here, *n_inliers = 0); n == 7 all 1; 8..14 LMedS; >= 15 RANSAC over 7-point
 *       samples drawn by cv::RNG(-1), at most 1000 iterations, adaptive stop.  pt1 / pt2: n x (x, y) float.
 *       No model found => mask all 0 (the reference leaves the mask uninitialised in that case).
 *   se2gpu_track_remove_outliers   = the whole member function: matches[i] (n1 entries, index into kps2 or -1) is set to
 *       -1 for the outliers; with fewer than 10 inliers every match is dropped and *n_inliers = 0.
 *   se2gpu_track_last_ransac       = {inliers, winning sample, winning model of that sample, iterations the reference's
 *       loop would have run} of the last call, for tracing. */
typedef struct se2gpu_track se2gpu_track;
int se2gpu_track_create(se2gpu_track** out);
void se2gpu_track_destroy(se2gpu_track* h);
int se2gpu_track_fundamental_mask(se2gpu_track* h, const float* pt1, const float* pt2, int n, uint8_t* mask,
                                  int* n_inliers);
int se2gpu_track_remove_outliers(se2gpu_track* h, const se2gpu_keypoint* kps1, int n1, const se2gpu_keypoint* kps2,
                                 int n2, int32_t* matches, int* n_inliers);
int se2gpu_track_last_ransac(const se2gpu_track* h, int info[4]);
/* The handle's calls run on its own stream, or on `hip_stream` (NULL -> its own stream again), which the caller keeps alive
 * and has to have drained before it changes streams.  se2gpu_track_sync waits for the stream in use. */
int se2gpu_track_set_stream(se2gpu_track* h, void* hip_stream);
void* se2gpu_track_stream(se2gpu_track* h);
int se2gpu_track_sync(se2gpu_track* h);

/* Loop verification: what both VerifyLoopClose of the reference run behind SearchByBoW (GlobalMapper.cpp:256-326 with
 * RemoveMatchOutlierRansac :1207-1248 and RemoveKPMatch :1251-1276; Localizer.cpp:394-431 with :571-612) for npairs pairs of
 * key frames at once.  Every pointer is device memory in the layouts of se2gpu_search_by_bow_batch_device; d_matches12 is the
 * array that call writes.  The x, y of d_kps are the positions tested (the reference passes keyPointsUn).
 * For pair p, a = pair_a[p], b = pair_b[p], counts clamped to 0..cap:
 *   raw matches   entries i < counts[a] of row p with a value in 0..counts[b]-1; every other entry counts as -1.  Their
 *                 points are taken in ascending i, the order of the reference's std::map<int,int>.
 *   filter        fewer than 10 raw matches: nothing survives (numMinMatch).  Otherwise the mask of cv::findFundamentalMat
 *                 exactly as se2gpu_track_fundamental_mask computes it for those points (LMedS for 10..14, RANSAC from 15
 *                 on, all 0 when no model exists).
 *   d_matches_good   row p = the input row with the non-survivors at -1, and -1 from counts[a] on
 *   d_matches_mp     the same, without the entries where has_mp[a][i] or has_mp[b][m] is 0 (RemoveKPMatch); may be NULL
 *   d_info[p * 8 ..] = {n_raw, n_good, n_good_mp, n_mps_a, path, best sample, best model, iterations}
 *                 n_good_mp: 0 without d_has_mp.   path: 0 skipped, 1 LMedS, 2 RANSAC.  The last three have the meaning
 *                 of se2gpu_track_last_ransac and are -1, -1, 0 on path 0.  n_mps_a (getAllObsMPs().size() in the reference's
 *                 ratio): d_num_mps[a] when d_num_mps is given, else the number of set flags among the first counts[a] of
 *                 has_mp[a], else 0.
 * A pair naming a frame outside 0..nframes-1 is a skipped pair without matches: rows of -1, info {0, 0, 0, 0, 0, -1, -1, 0}.
 * Nothing is indexed outside the arrays, whatever they hold.  The outputs must not overlap the inputs.
 * Asynchronous on the handle's stream: nothing is read back and nothing waits, so with se2gpu_track_set_stream(h,
 * se2gpu_matcher_stream(m)) the matcher's batch call and this one follow each other without the host in between.  (The first
 * call on a handle allocates the scratch and copies an 32 KiB table of random numbers to the device, which blocks.)  The
 * scratch - per pair 1000 x 27 doubles of models, 3000 scores, 7000 sample indices, 21 bytes per feature - lives in the
 * handle and is reused by the next call; it is capped at 64 MiB whatever npairs is (about 230 pairs at cap = 1024): a larger
 * batch runs as equal slices of at most that many pairs, one after the other on the same stream.
 * SE2GPU_ERR_INVALID: a NULL handle or required pointer, npairs / cap / nframes < 1, d_matches_mp without d_has_mp.
 * SE2GPU_ERR_CAPACITY: cap > 65536 or npairs > 65535, the limits of se2gpu_search_by_bow_batch_device.
 * The argument checks come first and use neither the handle nor a device. */
int se2gpu_track_loop_verify_batch_device(se2gpu_track* h,
                                          const se2gpu_keypoint* d_kps, const int32_t* d_counts, int cap, int nframes,
                                          const uint8_t* d_has_mp /* nframes*cap, may be NULL */,
                                          const int32_t* d_num_mps /* nframes, may be NULL */,
                                          const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs,
                                          const int32_t* d_matches12 /* npairs*cap */,
                                          int32_t* d_matches_good /* npairs*cap, out */,
                                          int32_t* d_matches_mp /* npairs*cap, out; may be NULL */,
                                          int32_t* d_info /* npairs*8, out */);
/* se2gpu_triangulate (below) on the workspace of the tracking thread: one packed upload / download, no allocation */
int se2gpu_track_triangulate(se2gpu_track* h, int n, const se2gpu_keypoint* kps_ref, const se2gpu_keypoint* kps_cur,
                             int n_cur, int32_t* match_idx, const uint8_t* has_observation, const float* P_ref,
                             const float* P_cur, const float* Ocam, float lower_depth, float upper_depth,
                             int min_degree, float* pos_out, uint8_t* good_parallax, int* n_good, int* n_tracked_old);

/* Track::removeOutliers (Track.cpp:308-344) and then Track::doTriangulate (Track.cpp:378-419) for npairs pairs (reference key
 * frame, current frame) at once: what Track::mTrack runs behind MatchByWindow on every frame.  Every d_ pointer is device
 * memory.  The frames are in the layouts of se2gpu_match_window_batch_device (d_kps_un, d_counts, cap, nframes), d_matches12 is
 * the array that call writes, and d_matched12 / d_local_pos are the arrays se2gpu_kf_correspd_batch_device reads, in its layouts;
 * d_kf_observed / d_view_pos are that call's tables (mViewMPs).
 *   d_Trc (npairs x 12)  rows 0-2 of cvu::inv(mFrame.Tcr), as se2gpu_kf_correspd_batch_device takes them; Ocam is column 3
 *   d_P   (npairs x 12)  Config::Kcam * Tcr.rowRange(0,3), formed by the caller as for se2gpu_track_triangulate
 *   P_ref (host, 12)     Config::PrjMtrxEye
 *   d_pair_flags         bit 0 set: the triangulation is skipped (Track.cpp:379-381, mFrame.id - mpKF->id < nMinFrames)
 * For pair p, a = pair_ref[p], b = pair_cur[p], counts clamped to 0..cap:
 *   raw matches   entries i < counts[a] of row p with a value in 0..counts[b]-1, in ascending i; every other entry counts as -1
 *   filter        the mask of cv::findFundamentalMat exactly as se2gpu_track_fundamental_mask computes it for those points (the
 *                 launches of se2gpu_track_loop_verify_batch_device, with its 64 MiB slices of scratch); with fewer than 10
 *                 inliers - always so below 10 raw matches - the whole row becomes -1 and the inlier count 0
 *   triangulation per i with a surviving match m, unless flag bit 0 is set:
 *                 kf_observed[a][i] set: local_pos = view_pos[a][i], counted as tracked old, good_prl = 0
 *                 else pos = cvu::triangulate(kps_un[a][i], kps_un[b][m], P_ref, P[p]) as se2gpu_track_triangulate forms it, bit
 *                 for bit; lower_depth <= pos.z <= upper_depth: local_pos = pos, good_prl = cvu::checkParallax(0, Ocam, pos,
 *                 min_degree); else the match becomes -1
 * Outputs, every word of them written for every (p, i < cap): d_matched12, d_local_pos (zero where the final match is -1, and
 * everywhere in a skipped pair), d_good_prl (0 everywhere in a skipped pair: the reference keeps the previous frame's flags
 * there, that state is the caller's).
 *   d_info[p * 8 ..] = {n_raw, n_inliers (nMatched of Track.cpp:134, 0 when dropped), n_tracked_old, n_good_prl (mnGoodPrl),
 *                 n_old_kp, path, n_depth_rejected, status}
 *                 n_old_kp: set bytes among the first counts[a] of kf_observed[a] (getSizeObsMP() of needNewKF), 0 without it
 *                 path: as in the loop verification (0 below 10 raw matches, 1 LMedS, 2 RANSAC)
 *                 status: 0 run, 1 a frame outside 0..nframes-1 (rows of -1, zeros), 2 fewer than 10 inliers, 3 triangulation
 *                 skipped by flag; the first that applies
 * Nothing is indexed outside the arrays, whatever they hold.  The outputs must not overlap the inputs.  A pair's outputs depend
 * on that pair only; they are the same in every run and wherever the pair stands in the batch (no floating-point or global
 * atomic).  Asynchronous on the handle's stream: nothing is uploaded besides kernel arguments, nothing is read back, nothing
 * waits; with se2gpu_track_set_stream(h, se2gpu_matcher_stream(m)) extract -> MatchByWindow -> this call -> findCorrespd follow
 * each other on one stream.  The first call on a handle allocates the scratch of the loop verification (and blocks as that
 * call's first does); later calls of the same or a smaller size allocate nothing.
 * SE2GPU_ERR_INVALID: a NULL handle or required pointer (d_kf_observed, d_view_pos and d_pair_flags may be NULL), d_kf_observed
 *   without d_view_pos, npairs / cap / nframes < 1, min_degree outside 1..4.
 * SE2GPU_ERR_CAPACITY: cap > 65536 or npairs > 65535, as se2gpu_track_loop_verify_batch_device.
 * The argument checks come first and use neither the handle nor a device. */
int se2gpu_track_frames_batch_device(se2gpu_track* h,
                                     const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap, int nframes,
                                     const uint8_t* d_kf_observed /* nframes*cap, may be NULL */,
                                     const float* d_view_pos /* nframes*cap*3; required with d_kf_observed */,
                                     const int32_t* d_pair_ref, const int32_t* d_pair_cur, int npairs,
                                     const float* d_Trc /* npairs*12 */, const float* d_P /* npairs*12 */,
                                     const uint8_t* d_pair_flags /* npairs, may be NULL */,
                                     const float* P_ref /* host, 12 */,
                                     const int32_t* d_matches12 /* npairs*cap, in */,
                                     float lower_depth, float upper_depth, int min_degree,
                                     int32_t* d_matched12 /* npairs*cap, out */, float* d_local_pos /* npairs*cap*3, out */,
                                     uint8_t* d_good_prl /* npairs*cap, out */, int32_t* d_info /* npairs*8, out */);

/* Localizer::DoLocalBA (/root/reference/src/Localizer.cpp:233-302) - SURVEY section 8(f).2: pose-only bundle adjustment of one
 * key frame against the fixed map points it observes, the whole optimize(iters) in one launch.
 *   pose12      = rotation row-major (9) then translation (3) of a rigid transform, x_c = R x_w + t (Tcw)
 *   se2gpu_plane_motion_prior  = addPlaneMotionSE3Expmap (src/optimizer.cpp:236-314): measurement = the pose with the body's
 *       roll, pitch and height removed (Tbc = Config::bTc), information = adj(Tbc)^T diag(xrot, yrot, 1e-4, 1e-4, 1e-4, z)
 *       adj(Tbc), vector order (rotation, translation); graph construction, runs on the host
 *   se2gpu_track_pose_ba       = VertexSE3Expmap + n EdgeProjectXYZ2UV (information inv_sigma2[i] * I, Huber huber_delta,
 *       single focal length f as addCamPara builds g2o::CameraParameters) + EdgeSE3ExpmapPrior(prior_meas, prior_info),
 *       Levenberg-Marquardt with g2o's policy; xyz: n x 3 world points, uv: n x 2 key-point positions.
 *       stats has the meaning it has for se2gpu_ba_optimize. */
int se2gpu_plane_motion_prior(const double* Tcw12, const double* Tbc12, double xrot_info, double yrot_info, double z_info,
                              double* meas12, double* info36);
int se2gpu_track_pose_ba(se2gpu_track* h, const double* Tcw12, const double* prior_meas12, const double* prior_info36, int n,
                         const double* xyz, const double* uv, const double* inv_sigma2, double f, double cx, double cy,
                         double huber_delta, int iters, double* Tcw_out12, se2gpu_ba_stats* stats);

/* Per-observation information matrices of Map::loadLocalGraph (/root/reference/src/Map.cpp:1024-1049), SURVEY §8f.1:
 *   Sigma = s_rot * J_r J_r^T + s_z * J_z J_z^T + sigma2 * I,   Omega = Sigma^-1       (2x2, FP64)
 *   J_r = (J_pi Rcw skew(lw - p))[:, 0:2],  J_z = -(J_pi Rcw)[:, 2],  J_pi from the stored camera-frame point lc.
 * Host buffers: lc, lw (E x 3 float: KeyFrame::mViewMPs[ftrIdx], MapPoint::getPos()), e_kf (E, index into the P
 * key frames), sigma2 (E float: mvLevelSigma2[octave]), Rcw (P x 9 float, row-major rotation of KeyFrame::Tcw),
 * twb_xy (P x 2 float: Twb.x, Twb.y), fx = Config::fxCam, xrot_info / z_info = Config::PLANEMOTION_XROT_INFO / _Z_INFO.
 * info_out: E x 4 doubles (row-major 2x2), ready for se2gpu_ba_add_edge_se2xyz. */
int se2gpu_ba_edge_information(int E, const float* lc, const float* lw, const int32_t* e_kf, const float* sigma2, int P,
                               const float* Rcw, const float* twb_xy, float fx, float xrot_info, float z_info,
                               double* info_out);

/* Multi-GPU (landmark-sharded) BA, SURVEY.md §8e: every rank holds all poses and a shard of the
 * landmarks (+ their edges); odometry edges live on one rank.  Once per LM trial the library calls
 *     allreduce(dev_ptr, count_doubles, hip_stream, user)
 * which must sum `count_doubles` FP64 values in place over all ranks, ordered on `hip_stream`
 * (RCCL ncclAllReduce(ncclDouble, ncclSum), or torch.distributed.all_reduce on a tensor that
 * aliases the buffer).  The fused buffer is [S (3P*3P) | bs (3P) | 4 scalars]; a second call
 * reduces the 4 trial scalars.  If `buffer` is non-NULL it must be a device allocation of at least
 * se2gpu_ba_reduce_buffer_doubles(h) doubles, used instead of an internal one (so the caller can
 * alias it with its own tensor).
 * Without a caller buffer the big exchange ships only what the dense solver reads: of row r of [S; bs^T] (r = 0 .. 3P)
 * the columns [0, 32 (r / 32 + 1)) - the lower-triangular 32 x 32 tiles and the rhs row - packed back to back;
 * se2gpu_ba_exchange_row gives the offset and length of a row in that packed buffer (host function, no device needed) and
 * se2gpu_ba_exchange_doubles(P) its total size.  With a caller buffer the rows 0 .. 3P of the rectangle are reduced in
 * place. */
typedef int (*se2gpu_allreduce_fn)(void* dev_ptr, size_t count_doubles, void* hip_stream, void* user);
size_t se2gpu_ba_reduce_buffer_doubles(se2gpu_ba* h, int P);
size_t se2gpu_ba_exchange_doubles(int P);
/* The same for an initialised handle: when the library re-orders the poses for the dense solve (nested dissection, padded
 * partitions - every rank of a sharded run chooses the same order from the merged block pattern, one extra small
 * all-reduce inside initialize) the packed exchange has the rows of THAT system; equal to se2gpu_ba_exchange_doubles(P)
 * in the natural order.  0 before initialize. */
size_t se2gpu_ba_exchange_doubles_h(const se2gpu_ba* h);
int se2gpu_ba_exchange_row(int row, size_t* offset, int* length);
int se2gpu_ba_set_allreduce(se2gpu_ba* h, se2gpu_allreduce_fn fn, void* user, void* buffer);
/* This handle holds landmark shard `rank` of `world` (rank 0 owns the odometry edges and the
 * lambda*I / fixed-pose identity terms, which must enter the sum exactly once). */
int se2gpu_ba_set_shard(se2gpu_ba* h, int rank, int world);

/* Native RCCL communicator (one process per GPU).  The library dlopen()s the system librccl.so.1 - it is NOT a link
 * dependency of single-GPU users - and calls ncclAllReduce(ncclDouble, ncclSum) in place on the handle's stream.
 * Rendezvous of the 128-byte ncclUniqueId is the caller's business (bench.py broadcasts it with torch.distributed
 * over gloo; a ROS deployment would use its own transport).  se2gpu_ba_set_comm = set_shard(rank, world) + an internal
 * all-reduce through this communicator. */
typedef struct se2gpu_comm se2gpu_comm;
int se2gpu_comm_unique_id(uint8_t id_out[128]);                       /* ncclGetUniqueId (rank 0) */
int se2gpu_comm_create(const uint8_t id[128], int rank, int world, se2gpu_comm** out);  /* ncclCommInitRank */
int se2gpu_comm_count(se2gpu_comm* c, int* nranks);                      /* ncclCommCount */
void se2gpu_comm_destroy(se2gpu_comm* c);
int se2gpu_comm_allreduce_sum_f64(se2gpu_comm* c, void* dev_ptr, size_t count, void* hip_stream);
int se2gpu_ba_set_comm(se2gpu_ba* h, se2gpu_comm* c);

/* Host-side landmark partition ("sharded by keyframe window"): owner[l] in [0, world) for the
 * L landmarks of a graph given by its edge lists.  Pure host code (no device needed). */
int se2gpu_ba_shard_landmarks(int L, int E, const int32_t* e_kf, const int32_t* e_lm, int world, int32_t* owner);

/* ------------------------------------------------------------------------------------------
 * DBoW2 vocabulary  -  se2lam::ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) on the device
 *   transform(features, bow, fv, levelsup)   Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1150-1216, 1241-1280
 *                                            (KeyFrame::ComputeBoW, src/KeyFrame.cpp:244-254; Localizer.cpp:195-205, 323-335)
 *   score(v1, v2)                            Thirdparty/DBoW2/DBoW2/ScoringObject.cpp
 *   the candidate loop of DetectLoopClose    src/GlobalMapper.cpp:201-254, src/Localizer.cpp:337-391
 *   create(training_features, k, L, ..)      Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:573-1020   (se2gpu_voc_train)
 * Every output equals the host mirror include/se2lam_amd/ORBVocabulary.h bit for bit: word ids, node ids, feature indices,
 * BowVector values and scores (all floating-point sums are added in ascending word id, as the mirror adds them).
 * Scoring / weighting constants are DBoW2's: scoring 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA,
 * 5 DOT_PRODUCT; weighting 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY.
 * ------------------------------------------------------------------------------------------ */
/* The tree on the device.  Immutable after creation: any number of contexts, data bases and threads may share one, as the
 * reference shares one ORBVocabulary between GlobalMapper and Localizer.  It must outlive everything created from it. */
typedef struct se2gpu_voc se2gpu_voc;
/* The records of the binary vocabulary file: `nodes` nodes including the root, which is node 0 (its entries are ignored);
 * parent[nodes], desc[nodes * 32], weight[nodes] (rounded to float, which is what the file stores), leaf[nodes].  Children
 * keep the order of their ids.  Refuses (SE2GPU_ERR_INVALID) exactly what ORBVocabulary::loadFromBinaryFile refuses - the
 * check is the same code (include/se2lam_amd/VocabularyTree.h): a header out of range, a parent that does not precede its
 * child, a childless node that is not a leaf. */
int se2gpu_voc_create(int k, int L, int scoring, int weighting, int nodes, const int32_t* parent, const uint8_t* desc,
                      const double* weight, const uint8_t* leaf, se2gpu_voc** out);
/* the file TemplatedVocabulary::saveToBinaryFile writes; a missing or truncated file is refused as well */
int se2gpu_voc_load(const char* path, se2gpu_voc** out);
void se2gpu_voc_destroy(se2gpu_voc* v);
int se2gpu_voc_words(const se2gpu_voc* v);      /* size(); the accessors return SE2GPU_ERR_INVALID for a NULL handle */
int se2gpu_voc_nodes(const se2gpu_voc* v);      /* including the root */
int se2gpu_voc_k(const se2gpu_voc* v);
int se2gpu_voc_L(const se2gpu_voc* v);
int se2gpu_voc_scoring(const se2gpu_voc* v);
int se2gpu_voc_weighting(const se2gpu_voc* v);
/* Every se2gpu_voc - loaded, created or trained - keeps its records in host memory as well (about 60 bytes per node, 65 MB
 * for a vocabulary of ORBvoc's size), which is what the two calls below read. */
/* the records back, in the layout se2gpu_voc_create takes (the root at index 0, weights as the file's floats widened);
 * SE2GPU_ERR_CAPACITY when the buffers hold fewer than se2gpu_voc_nodes entries */
int se2gpu_voc_export(const se2gpu_voc* v, int cap_nodes, int32_t* parent, uint8_t* desc, double* weight, uint8_t* leaf);
/* the file TemplatedVocabulary::saveToBinaryFile writes (and se2gpu_voc_load reads) */
int se2gpu_voc_save(const se2gpu_voc* v, const char* path);

/* Training - TemplatedVocabulary::create (TemplatedVocabulary.h:573-1020): hierarchical k-means++ over the descriptors of
 * nframes documents, on the device, level by level (csrc/voc_train.hip).  The algorithm, its draws and its documented
 * deviations from the reference are specified in include/se2lam_amd/VocabularyTrain.h; the result equals the host mirror
 * ORBVocabulary::create bit for bit, statistics included.  desc: nframes * cap * 32 bytes, counts: nframes ints clamped to
 * 0..cap - the layout se2gpu_orb_extract_batch_device writes and se2gpu_bow_transform_batch_device reads; host memory, or
 * device memory when on_device != 0 (desc then 16-byte aligned).  Refused with SE2GPU_ERR_INVALID: k outside 2..32, L outside
 * 1..10, a scoring / weighting se2gpu_voc_create refuses, no descriptor at all, a document with more than 4096 descriptors.
 * Synchronous, on a stream of its own; every scratch buffer is released before it returns. */
typedef struct {
    int32_t k, L, scoring, weighting, max_iters; /* max_iters 0 = 1000 */
    uint64_t seed;
} se2gpu_voc_train_params;
typedef struct {
    int32_t nodes, words, kmeans_nodes, trivial_nodes, lloyd_iters_total, lloyd_iters_max, short_seeded_nodes, empty_clusters,
        capped_nodes, zero_weight_words;
} se2gpu_voc_train_stats;
int se2gpu_voc_train(const se2gpu_voc_train_params* params, const uint8_t* desc, const int32_t* counts, int cap, int nframes,
                     int on_device, se2gpu_voc** out, se2gpu_voc_train_stats* stats /* may be NULL */);
/* per-kernel times of the training calls that start after this call (HIP events around every launch: serialises that call).
 * The switch is process-wide; every training call times into a table of its own and publishes it when it ends, so calls on
 * several threads do not disturb each other.  _get walks the table of the call that ended last, SE2GPU_ERR_INVALID past its
 * end. */
int se2gpu_voc_train_profile(int enable);
int se2gpu_voc_train_profile_get(int idx, const char** name, double* ms, int64_t* launches);

/* A per-thread context: its stream and scratch for batches of up to max_batch frames of up to max_features (<= 4096)
 * features.  Not thread-safe; several contexts may share one vocabulary. */
typedef struct se2gpu_bow se2gpu_bow;
int se2gpu_bow_create(const se2gpu_voc* voc, int max_features, int max_batch, se2gpu_bow** out);
void se2gpu_bow_destroy(se2gpu_bow* h);
int se2gpu_bow_set_stream(se2gpu_bow* h, void* hip_stream);  /* NULL -> the context's own stream */
int se2gpu_bow_sync(se2gpu_bow* h);
void* se2gpu_bow_stream(se2gpu_bow* h);
/* transform(.., levelsup) of nframes frames whose descriptors lie where se2gpu_orb_extract_batch_device wrote them
 * (d_desc: nframes * cap * 32 bytes, 16-byte aligned; d_counts: nframes ints, clamped to 0..cap).  Outputs of frame f, all
 * device memory: the BowVector d_bow_word (u32) / d_bow_value (f64) from f * cap, ascending word id, d_bow_n[f] words; the
 * FeatureVector as the CSR se2gpu_search_by_bow takes (se2gpu_search_by_bow_batch_device reads it where it lies) - d_fv_nodes from f * cap (ascending node ids of the file), d_fv_ptr
 * from f * (cap + 1), d_fv_idx from f * cap (ascending within a node), d_fv_nn[f] nodes.  A feature on a word of weight 0
 * is in neither vector; the node of a feature is its ancestor at level L - levelsup (the root when that is not positive,
 * the leaf when the leaf lies above that level); an empty frame gives empty vectors.  Asynchronous on the context's stream. */
int se2gpu_bow_transform_batch_device(se2gpu_bow* h, const uint8_t* d_desc, const int32_t* d_counts, int cap, int nframes,
                                      int levelsup, uint32_t* d_bow_word, double* d_bow_value, int32_t* d_bow_n,
                                      int32_t* d_fv_nodes, int32_t* d_fv_ptr, int32_t* d_fv_idx, int32_t* d_fv_nn);
/* the same for one frame with host buffers (n descriptors; bow_*, fv_nodes, fv_idx: n entries, fv_ptr: n + 1); synchronous */
int se2gpu_bow_transform(se2gpu_bow* h, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word, double* bow_value,
                         int* nb, int32_t* fv_nodes, int32_t* fv_ptr, int32_t* fv_idx, int* nn);

/* The key frames' BowVectors, resident on the device, in insertion order.  One thread at a time; KL scoring is refused at
 * create (SE2GPU_ERR_INVALID): it needs the host's log() bit for bit and nothing in se2lam uses it. */
typedef struct se2gpu_bowdb se2gpu_bowdb;
int se2gpu_bowdb_create(const se2gpu_voc* voc, se2gpu_bowdb** out);
void se2gpu_bowdb_destroy(se2gpu_bowdb* db);
/* host buffers: n ascending word ids and their values, as transform() leaves them; synchronous */
int se2gpu_bowdb_add(se2gpu_bowdb* db, int kf_id, const uint32_t* word, const double* value, int n);
/* a frame's slice of se2gpu_bow_transform_batch_device's output where it lies: d_word / d_value point at the slice (cap
 * entries), d_n at its d_bow_n entry.  Asynchronous on the context's stream, after the transform that writes the slice. */
int se2gpu_bowdb_add_device(se2gpu_bowdb* db, se2gpu_bow* ctx, int kf_id, const uint32_t* d_word, const double* d_value,
                            const int32_t* d_n, int cap);
/* Map::pruneRedundantKF deletes key frames: drops the first entry with that id; the later entries move up one place */
int se2gpu_bowdb_remove(se2gpu_bowdb* db, int kf_id);
int se2gpu_bowdb_size(const se2gpu_bowdb* db);
/* scores_out[i] (host, size() doubles, may be NULL) = score(query, entry i) for every entry, and the candidate
 * DetectLoopClose would keep: entries with abs(kf_id - cur_kf_id) < min_kfid_offset are skipped, the best starts at 0 and
 * an entry replaces it when its score is strictly greater - so *best_entry is the first entry at the maximal score, or -1
 * (with *best_kf_id = -1, *best_score = 0) when no score is above 0.  The comparison with the minimal accepted score stays
 * with the caller.  The query (n ascending words, n <= the context's max_features) is read from host memory, or from
 * device memory when query_on_device != 0.  Synchronous. */
int se2gpu_bowdb_query(se2gpu_bowdb* db, se2gpu_bow* ctx, const uint32_t* word, const double* value, int n,
                       int query_on_device, int cur_kf_id, int min_kfid_offset, double* scores_out, int* best_entry,
                       int* best_kf_id, double* best_score);

/* ------------------------------------------------------------------------------------------
 * Timing helpers for bench.py: HIP events on the stream the kernels are launched on.
 * ------------------------------------------------------------------------------------------ */
typedef struct se2gpu_timer se2gpu_timer;
int se2gpu_timer_create(se2gpu_timer** out);
void se2gpu_timer_destroy(se2gpu_timer* t);
int se2gpu_timer_start(se2gpu_timer* t, void* hip_stream);
int se2gpu_timer_stop(se2gpu_timer* t, void* hip_stream);
int se2gpu_timer_elapsed_ms(se2gpu_timer* t, float* ms);  /* synchronises on the stop event */
void* se2gpu_orb_stream(se2gpu_orb* h);
void* se2gpu_matcher_stream(se2gpu_matcher* h);
void* se2gpu_ba_stream(se2gpu_ba* h);
/* Per-kernel accumulated device time (ms) / launch count since the last reset, measured with HIP
 * events around every launch when profiling is enabled on the handle (adds sync overhead). */
int se2gpu_ba_profile(se2gpu_ba* h, int enable);
int se2gpu_ba_profile_get(se2gpu_ba* h, int idx, const char** name, double* ms, int64_t* launches);
/* FAST score kernel selection (SE2GPU_ORB_SCORE = auto | dense | sparse, default auto): info[0] = kernel the next batch
 * would use (0 = every pixel, 1 = compass pre-test + candidates only), info[1] = last measured candidate density * 1e6, -1
 * before the first measurement.  Both kernels produce the same plane. */
int se2gpu_orb_score_kernel(se2gpu_orb* h, int info[2]);
int se2gpu_orb_profile(se2gpu_orb* h, int enable);
int se2gpu_orb_profile_get(se2gpu_orb* h, int idx, const char** name, double* ms, int64_t* launches);

/* Raw device memory helpers so a non-torch caller (and the tests) can stage device buffers. */
int se2gpu_malloc(void** dev_ptr, size_t bytes);
int se2gpu_free(void* dev_ptr);
int se2gpu_memcpy_h2d(void* dst, const void* src, size_t bytes);
int se2gpu_memcpy_d2h(void* dst, const void* src, size_t bytes);
int se2gpu_device_synchronize(void);
int se2gpu_set_device(int ordinal);
/* Streaming helpers (the camera thread's upload path: pinned staging, asynchronous copies on a stream of its own,
 * cross-stream ordering through the stop event of a timer): what bench.py's `orb.streaming` leg is built from. */
int se2gpu_host_alloc(void** host_ptr, size_t bytes);   /* pinned */
int se2gpu_host_free(void* host_ptr);
int se2gpu_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* hip_stream);
int se2gpu_memcpy_d2h_async(void* dst, const void* src, size_t bytes, void* hip_stream);
int se2gpu_stream_create(void** hip_stream_out);
int se2gpu_stream_destroy(void* hip_stream);
int se2gpu_stream_synchronize(void* hip_stream);
int se2gpu_timer_stream_wait(se2gpu_timer* t, void* hip_stream);  /* hip_stream waits for the timer's stop event */

#ifdef __cplusplus
}
#endif
#endif /* SE2GPU_H */
