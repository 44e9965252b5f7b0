/* vio_posegraph.h -- C ABI of the loop-closure slice of pose_graph.
 *
 * The reference's pose_graph nodelet (pose_graph/src) builds a KeyFrame per estimator keyframe, asks DBoW2 for a loop candidate
 * (PoseGraph::detectLoop, pose_graph.cpp:308 = vio_pg_detect_loop below; the vocabulary blob is missing from the reference tree, the caller
 * supplies the file), verifies it (KeyFrame::findConnection) and, on success, hands the estimator the match list (Estimator::setReloFrame =
 * vio_set_relo_frame in vio_abi.h) and runs the 4-DoF pose-graph optimisation.  Each entry point names the reference interface it replaces.
 * Descriptor extraction and matching run as HIP kernels on the current device (no CPU fallback: VIO_EDEVICE without a GPU); the geometric
 * verification and the pose-graph optimisation are per-keyframe host code, like the reference's.  Plain C types, caller-owned buffers.
 */
#ifndef VIO_POSEGRAPH_H
#define VIO_POSEGRAPH_H
#include <stdint.h>

#include "vio_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* KeyFrame::computeWindowBRIEFPoint + KeyFrame::computeBRIEFPoint (pose_graph/src/keyframe/keyframe.cpp:80-124) with DVision::BRIEF::compute
 * (ThirdParty/DVision/BRIEF.cpp): GaussianBlur(9x9, sigma 2) of `gray` (cfg->height x cfg->width, u8, host), 256-bit BRIEF descriptors of the
 * n_win window points win_uv[n_win][2] (pixel coordinates of the tracked features) into win_desc[n_win][4]; cv::FAST(image, fast_threshold,
 * NMS) keypoints of the raw image in row-major order into kp_xy[cap][2], their descriptors into kp_desc[cap][4] and their normalised
 * coordinates (m_camera->liftProjective) into kp_norm[cap][2].  pattern1024 = x1[256] y1[256] x2[256] y2[256] of BRIEF_PATTERN_FILE
 * (support_files/brief_pattern.yml).  Returns the number of keypoints found (may exceed cap: only cap are written) or a negative status. */
int vio_pg_describe(const vio_config *cfg, const uint8_t *gray, int n_win, const float *win_uv, const int32_t *pattern1024, int fast_threshold,
                    uint64_t *win_desc, int cap, float *kp_xy, uint64_t *kp_desc, float *kp_norm);
/* vio_pg_describe with the keypoints lifted through a camera model (vio_abi.h's vio_camera, as KeyFrame::computeBRIEFPoint lifts them through
 * m_camera): kp_norm = (x / z, y / z) of liftProjective.  cfg still gives the image size. */
int vio_pg_describe_camera(const vio_config *cfg, const vio_camera *cam, const uint8_t *gray, int n_win, const float *win_uv,
                           const int32_t *pattern1024, int fast_threshold, uint64_t *win_desc, int cap, float *kp_xy, uint64_t *kp_desc,
                           float *kp_norm);

/* KeyFrame::searchByBRIEFDes / searchInAera / HammingDis (keyframe.cpp:126-169, 530): for each of the n window descriptors the FIRST old
 * descriptor with the smallest Hamming distance below 128; best_index[i] = its index if the distance is below 80, else -1. */
int vio_pg_match(const uint64_t *win_desc, int n, const uint64_t *old_desc, int m, int32_t *best_index, int32_t *best_dist);

/* KeyFrame::findConnection (keyframe.cpp:252-528) after the descriptor search, incl. KeyFrame::PnPRANSAC (:195-250).  Current keyframe: n
 * window points -- world point pt3d[n][3], feature id pt_id[n], match[n] from vio_pg_match against the old keyframe -- and its origin_vio
 * pose (vio_T[3], vio_R[9] row-major); old_norm[m][2] = the old keyframe's normalised keypoints; qic[9], tic[3] = the camera extrinsic.
 * Returns 1 if more than min_loop_num (MIN_LOOP_NUM = 25) matches survive the PnP RANSAC and |relative yaw| < 30 deg, |relative t| < 20 m:
 * loop_info[8] = relative_t(3), relative_q(w, x, y, z), relative_yaw (deg); match_points[n_match][3] = (x, y of the old normalised keypoint,
 * feature id) in ascending window order -- the list pose_graph publishes for Estimator::setReloFrame (:491-520; pass it with the OLD keyframe's
 * pose to vio_set_relo_frame).  0 = no loop; negative = status.  pnp_T[3], pnp_R[9]: PnP_T_old / PnP_R_old (diagnostics, may be NULL). */
int vio_pg_find_connection(int n, const float *pt3d, const double *pt_id, const int32_t *match, const float *old_norm, const double *vio_T,
                           const double *vio_R, const double *qic, const double *tic, int min_loop_num, double *loop_info, double *match_points,
                           int32_t *n_match, double *pnp_T, double *pnp_R);

/* PoseGraph::optimize4DoF (pose_graph/src/pose_graph/pose_graph.cpp:410-581; residuals pose_graph.h:102-256) over the n keyframes from the
 * earliest looped one to the current one, in list order: t[n][3], R[n][9] = their VIO poses, sequence[n], loop_to[n] = local index of the loop
 * partner or -1, loop_info[n][8].  Node 0 and the nodes of sequence 0 are held constant; sequential edges to the 1..4 previous keyframes of the
 * same sequence, loop edges under HuberLoss(0.1), yaw + translation free, five Levenberg-Marquardt iterations.  Writes the optimised poses
 * t_out[n][3], R_out[n][9] and drift[4] = (yaw_drift deg, t_drift(3)) of the newest keyframe (:547-553). */
int vio_pg_optimize4dof(int n, const double *t, const double *R, const int32_t *sequence, const int32_t *loop_to, const double *loop_info,
                        double *t_out, double *R_out, double *drift);

/* PoseGraph::optimize6DoF (pose_graph.cpp:583-740; RelativeRTError pose_graph.h:256-320), the `imu: 0` variant: full poses (quaternion with
 * ceres::QuaternionParameterization + translation), same node / edge selection as optimize4DoF, edges = RelativeRTError(relative t, relative q,
 * t_var 0.1, q_var 0.01) with the loop edges (loop_info[0..2] = relative t, [3..6] = relative q (w, x, y, z)) under HuberLoss(0.1), five
 * Levenberg-Marquardt iterations.  drift12 = r_drift (9, row-major) = R_cur R_vio^T, t_drift (3) = t_cur - r_drift t_vio (:717-721). */
int vio_pg_optimize6dof(int n, const double *t, const double *R, const int32_t *sequence, const int32_t *loop_to, const double *loop_info,
                        double *t_out, double *R_out, double *drift12);

/* ---- place recognition: BriefVocabulary + BriefDatabase of PoseGraph (pose_graph.h:83-84; vendored DBoW2 under pose_graph/src/ThirdParty) ----
 * The tree walk of every descriptor runs as a HIP kernel (no CPU fallback); bag-of-words vector, inverted file and L1 query are per-keyframe
 * host code.  Only L1_NORM scoring (what brief_k10L6.bin uses) is supported; all four weightings are.  The reference tree does not contain the
 * vocabulary blob (support_files/brief_k10L6.bin, .MISSING_LARGE_BLOBS): the caller supplies the file. */
typedef struct vio_pg_voc vio_pg_voc;
/* PoseGraph::loadVocabulary (pose_graph.cpp:44-47) = BriefVocabulary(path) -> TemplatedVocabulary::loadBin (TemplatedVocabulary.h:1509-1561) on the
 * file format of VINSLoop::Vocabulary::deserialize (ThirdParty/VocabularyBinary.{hpp,cpp}): 6 x int32 (k, L, scoringType, weightingType, nNodes,
 * nWords), nNodes x {int32 nodeId, int32 parentId, double weight, uint64 descriptor[4]}, nWords x {int32 nodeId, int32 wordId};
 * db.setVocabulary(*voc, false, 0) (no direct index).  NULL on failure (vio_last_error). */
vio_pg_voc *vio_pg_voc_load(const char *path);
/* the same from arrays (tests, vocabularies kept in another container): node i = (node_id[i], parent_id[i], weight[i], desc[i][4]) in file order */
vio_pg_voc *vio_pg_voc_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *node_id, const int32_t *parent_id,
                              const double *weight, const uint64_t *desc, int n_words, const int32_t *word_node, const int32_t *word_id);
void vio_pg_voc_destroy(vio_pg_voc *v);
/* out7 = k, L, scoring, weighting, nodes, words, database entries */
int vio_pg_voc_info(const vio_pg_voc *v, int32_t *out7);
/* TemplatedVocabulary::transform(feature, word_id, weight) (TemplatedVocabulary.h:1217-1260) for n descriptors desc[n][4] */
int vio_pg_voc_transform(vio_pg_voc *v, const uint64_t *desc, int n, int32_t *word_id, double *word_weight);
/* TemplatedVocabulary::transform(features, BowVector) (:1065-1122): ascending word ids and L1-normalised values; returns the vector's size */
int vio_pg_voc_bow(vio_pg_voc *v, const uint64_t *desc, int n, int cap, int32_t *word_id, double *value);
/* BriefDatabase::add (TemplatedDatabase.h:408-475; PoseGraph::addKeyFrameIntoVoc, pose_graph.cpp:395-408): returns the entry id (>= 0) */
int vio_pg_db_add(vio_pg_voc *v, const uint64_t *desc, int n);
/* BriefDatabase::query -> queryL1 (TemplatedDatabase.h): entries with id < max_id (or max_id == -1) and, as upstream, the newest entry; best
 * first, at most max_results (> 0), scores in [0, 1].  Ties are ordered by entry id (upstream: std::sort, unspecified).  Returns the count. */
int vio_pg_db_query(vio_pg_voc *v, const uint64_t *desc, int n, int max_results, int max_id, int32_t *ids, double *scores);
/* PoseGraph::detectLoop (pose_graph.cpp:308-393) for the keyframe's FAST-keypoint descriptors (kp_desc of vio_pg_describe): query(4,
 * frame_index - 50), add, then the score gates (best > 0.05 and another > 0.015, frame_index > 50) and the smallest candidate id.
 * *loop_index = that id or -1; ids4 / scores4 / n_ret (each may be NULL) = the query's results.  Returns a status. */
int vio_pg_detect_loop(vio_pg_voc *v, const uint64_t *desc, int n, int frame_index, int32_t *loop_index, int32_t *ids4, double *scores4,
                       int32_t *n_ret);

/* ---- the batch: one keyframe database per sequence, resident on the device (pg_batch.hip) ----
 * PoseGraph::detectLoop plus the descriptor search of KeyFrame::findConnection for every sequence of a batch in one chain of launches on a
 * stream of the batch's own: tree walk, bag-of-words vector, database score, top-4 and gates, append, search against the resident candidate.
 * A step allocates nothing, waits once (at its end) and copies one block of results back; the only host state is one entry counter per
 * sequence.  Every number equals what vio_pg_describe / vio_pg_detect_loop / vio_pg_match give for the same keyframes, bit for bit (the
 * kernels share their bodies, the floating-point sums keep the reference's order).  The geometric verification (vio_pg_find_connection) and
 * the optimisers stay per-keyframe host code, run by the caller for the sequences that report a candidate.
 *
 * Storage: per sequence one arena of arena_keypoints slots (descriptor 32 B, normalised and pixel keypoint 8 B each, bag-of-words word 4 B
 * and value 8 B: 60 B per slot) that the entries fill back to back, and max_keyframes + 1 offsets.  An entry takes as many slots as it keeps
 * keypoints (its bag-of-words vector is never longer).  frame_index of a sequence = its entry counter: every mode-1 or mode-2 step adds exactly
 * one entry. */
typedef struct vio_pg_batch vio_pg_batch;

/* S sequences; per sequence at most max_keyframes entries, max_keypoints (<= 8192) FAST keypoints and max_window window points per keyframe.
 * voc is borrowed (must outlive the batch; only its tree is used, its own database is untouched); pattern1024 as in vio_pg_describe.  All
 * device memory is allocated here.  vio_pg_batch_create sizes every arena for the worst case (max_keyframes x max_keypoints slots);
 * vio_pg_batch_create_arena takes the slots per sequence (>= max_keypoints).  NULL on failure (vio_last_error). */
vio_pg_batch *vio_pg_batch_create(const vio_config *cfg, vio_pg_voc *voc, int S, int max_keyframes, int max_keypoints, int max_window,
                                  const int32_t *pattern1024, int fast_threshold);
vio_pg_batch *vio_pg_batch_create_arena(const vio_config *cfg, vio_pg_voc *voc, int S, int max_keyframes, int max_keypoints, int max_window,
                                        const int32_t *pattern1024, int fast_threshold, int64_t arena_keypoints);
void vio_pg_batch_destroy(vio_pg_batch *b);
int  vio_pg_batch_set_camera(vio_pg_batch *b, int seq, const vio_camera *cam);      /* default: cfg's pinhole, like vio_pg_describe */
int  vio_pg_batch_reset_seq(vio_pg_batch *b, int seq);                              /* empty that sequence's database */

/* per-sequence result of one step, [S] of them, host */
typedef struct vio_pg_step_out {
    int32_t status;        /* VIO_OK, VIO_ECAPACITY (max_keyframes entries, or the arena has no room for this keyframe: nothing changed for this
                              sequence, no query is made: n_bow = n_ret = n_match = 0, loop_index = -1), or mode 0: the whole struct untouched */
    int32_t entry;         /* id of the entry added = that sequence's frame_index (VIO_ECAPACITY: the number of entries) */
    int32_t n_kp;          /* keypoints found (may exceed max_keypoints: only max_keypoints are kept, as vio_pg_describe with cap) */
    int32_t n_bow;         /* size of the bag-of-words vector */
    int32_t n_ret;         /* results of query(4, frame_index - 50); 0 in mode 2 */
    int32_t ids4[4];
    double  scores4[4];
    int32_t loop_index;    /* detectLoop's decision, -1 = none */
    int32_t n_match;       /* window descriptors with best_index != -1 against entry loop_index (0 when loop_index == -1) */
} vio_pg_step_out;

/* core: descriptors given.  mode[S]: 0 = no keyframe for this sequence this step, 1 = detectLoop (query, then add),
 * 2 = addKeyFrameIntoVoc (add only).  kp_desc [S][max_keypoints][4], kp_norm [S][max_keypoints][2], n_kp [S];
 * win_desc [S][max_window][4], n_win [S].  best_index / best_dist [S][max_window] and old_norm [S][max_window][2]
 * (the candidate's normalised keypoint at best_index, 0 where best_index is -1; gathered on the device) are written for rows < n_win of
 * sequences with loop_index != -1, and no other row is touched.  on_device != 0: every array except mode, n_kp, n_win and out is an HBM
 * address.  The pixel keypoints of entries added through this call are 0.  VIO_EINVAL (nothing launched, nothing changed): NULL handle or
 * array, a mode above 2, n_kp outside 0 .. max_keypoints or n_win outside 0 .. max_window for a sequence whose mode is not 0. */
int vio_pg_batch_step_desc(vio_pg_batch *b, const uint8_t *mode, const int32_t *n_kp, const uint64_t *kp_desc, const float *kp_norm,
                           const int32_t *n_win, const uint64_t *win_desc, int on_device, vio_pg_step_out *out,
                           int32_t *best_index, int32_t *best_dist, float *old_norm);

/* from images: gray [S][H][W] (the layout of vio_feed), win_uv [S][max_window][2] (u, v of kf_points from vio_publish_all).
 * = batched vio_pg_describe(_camera) into the batch's own buffers (the keypoint counts stay on the device), then the step above. */
int vio_pg_batch_step(vio_pg_batch *b, const uint8_t *mode, const uint8_t *gray, const int32_t *n_win, const float *win_uv, int on_device,
                      vio_pg_step_out *out, int32_t *best_index, int32_t *best_dist, float *old_norm);

/* read one stored entry back (tests, savePoseGraph): counts2 = n_kp kept, n_bow; kp_xy [n_kp][2], kp_desc [n_kp][4], kp_norm [n_kp][2],
 * bow_word / bow_value [n_bow]; any pointer may be NULL.  VIO_EINVAL for an entry that does not exist. */
int vio_pg_batch_get_entry(vio_pg_batch *b, int seq, int entry, int32_t *counts2, float *kp_xy, uint64_t *kp_desc, float *kp_norm,
                           int32_t *bow_word, double *bow_value);
int vio_pg_batch_info(vio_pg_batch *b, int32_t *entries /*[S]*/);
/* device time of the kernels of the last step in milliseconds (HIP events recorded on the batch's stream when timing is on; off by default,
 * the events cost a few microseconds each): ms8 = describe (blur, FAST, BRIEF, lift), tree walk, bag-of-words vector, database score,
 * top-4 / gates / append, match, result copy, whole chain.  tools/pg_batch_bench.py reads them. */
int vio_pg_batch_set_timing(vio_pg_batch *b, int on);
int vio_pg_batch_last_timing(vio_pg_batch *b, float *ms8);

/* test entry: the blurred image alone */
int vio_pg_stage_blur(const uint8_t *gray, int width, int height, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
