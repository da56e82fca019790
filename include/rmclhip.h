/*
 * rmclhip.h -- C ABI of librmclhip.so: the MI355X (gfx950) implementation of
 * RMCL / MICP-L's ray-casting-correspondence + pose-correction hot path.
 *
 * This is the drop-in boundary.  Every entry point names the
 * reference interface it replaces (paths relative to the uos/rmcl tree).  The
 * C++ adapters in include/rmcl_hip/ present it with the reference's class
 * shapes (Correspondences_<MemT>, SensorUpdater<MemT>); INTEGRATION.md shows the
 * reference-side glue.
 *
 * Conventions
 *  - plain pointers + sizes, no C++ / torch types; all structs are PODs with the
 *    reference's in-memory layouts (rmagine::Transform = {Quaternion{x,y,z,w},
 *    Vector{x,y,z}, uint32 stamp} = 32 B, pinned by
 *    rmcl_ros/src/nodes/rmcl_localization.cpp:245-249).
 *  - every function returns rmclhip_status (0 = OK) and never throws; the text
 *    of the last error on the calling thread is rmclhip_last_error().
 *    (The reference throws std::runtime_error -- micp_localization.cpp:613,
 *    PCDSensorUpdaterOptix.cpp:179-192 -- the C++ adapters rethrow.)
 *  - there is NO CPU fallback: without a HIP device every compute call fails
 *    with RMCLHIP_ERR_NO_DEVICE.
 *  - a handle is thread-compatible (no concurrent calls on one handle); each
 *    rcc / pf handle owns one HIP stream; calls are synchronous on return unless
 *    suffixed _async.
 *  - pointers suffixed _dev are device pointers (hipMalloc'd, e.g. a torch
 *    tensor's data_ptr()); all other pointers are host memory.
 */
#ifndef RMCLHIP_H
#define RMCLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMCLHIP_VERSION_MAJOR 0
#define RMCLHIP_VERSION_MINOR 1

typedef int rmclhip_status;
enum {
  RMCLHIP_OK = 0,
  RMCLHIP_ERR_INVALID = 1,    /* bad argument / state (reference: std::runtime_error) */
  RMCLHIP_ERR_NO_DEVICE = 2,  /* no HIP device: the product has no CPU path */
  RMCLHIP_ERR_HIP = 3,        /* a HIP runtime call failed (reference: RM_CUDA_CHECK throw) */
  RMCLHIP_ERR_NOMEM = 4,
  RMCLHIP_ERR_UNSUPPORTED = 5
};

/* ---- PODs ------------------------------------------------------------------ */
typedef struct { float x, y, z; } rmclhip_vec3;
typedef struct { float x, y, z, w; } rmclhip_quat;
/* rmagine::Transform (rmcl_localization.cpp:245-249) */
typedef struct { rmclhip_quat R; rmclhip_vec3 t; uint32_t stamp; } rmclhip_transform;
typedef struct { float min, inc; uint32_t size; } rmclhip_discrete_interval;
typedef struct { float min, max; } rmclhip_interval;
/* rmagine::SphericalModel; field meaning pinned by rmcl_ros/src/util/conversions.cpp:22-34
 * (phi = vertical/rows/height, theta = horizontal/cols/width) */
typedef struct {
  rmclhip_discrete_interval phi;
  rmclhip_discrete_interval theta;
  rmclhip_interval range;
} rmclhip_spherical_model;
/* rmagine::CrossStatistics (members pinned by micp_localization.cpp:87-105,934,1010-1011).
 * covariance is row-major, C(r,c) = 1/n sum (m_i - model_mean)_r (d_i - dataset_mean)_c */
typedef struct {
  rmclhip_vec3 dataset_mean;
  rmclhip_vec3 model_mean;
  float covariance[9];
  uint32_t n_meas;
} rmclhip_cross_statistics;
/* rmagine::Gaussian1D + rmcl::ParticleAttributes (ParticleAttributes.hpp:18-34), 36 B */
typedef struct { float mean, sigma; uint32_t n_meas; } rmclhip_gaussian1d;
typedef struct { rmclhip_gaussian1d likelihood; float state_sigma[6]; } rmclhip_particle_attributes;
/* rmcl::RangeMeasurement (RangeMeasurement.hpp:10-21), 64 B; cov row-major */
typedef struct { rmclhip_vec3 orig, dir; float range; float cov[9]; } rmclhip_range_measurement;
/* sensor_update.* parameters, defaults PCDSensorUpdaterEmbree.cpp:122-134
 * (== optix/EvaluationDataOptix.hpp:62-81 minus pointers) */
typedef struct {
  float dist_sigma;                 /* 2.0; >= 1e-10f (rmclhip_pf_set_params refuses less: the peak eval 1 / sqrt(2 pi sigma^2)
                                     *     must stay below 2^32, the top of the update's fixed-point accumulators) */
  float real_hit_sim_miss_error;    /* 100  */
  float real_miss_sim_hit_error;    /* 100  */
  float real_miss_sim_miss_error;   /* 0    */
  rmclhip_interval sensor_range;    /* [0.05, 80] */
  uint32_t max_n_meas;              /* MAX_N_MEAS = 10000, ParticleAttributes.hpp:34 */
  uint32_t correspondence_type;     /* 0 = RCC, the hybrid SURVEY.md App. B.1 recommends: UNIT face normals (as the OptiX
                                     *     program and rmagine's simulators) with the Embree updater's ray rules
                                     *     (tfar = inf, sim hit needs t > sensor_range.min);
                                     * 1 = CPC (evaluate_cpc, :88-95);
                                     * 2 = RCC exactly as PCDSensorUpdaterEmbree.cpp:18-86: like 0 but the error is taken
                                     *     against Embree's un-normalised rayhit.hit.Ng = cross(v2-v0, v0-v1), i.e. it scales
                                     *     with twice the triangle's area;
                                     * 3 = RCC exactly as optix/BeamEvaluateProgram.cu:15-130: unit normals, optixTrace
                                     *     tmax = 1e4, every hit is a sim hit (no sensor_range.min test) */
} rmclhip_pf_params;

/* The surface constraint of the motion update (rmclhip_pf_set_surface / rmclhip_pf_constrain_to_surface below state the rule);
 * rmclhip_surface_params_default fills the values in brackets. */
typedef struct {
  uint32_t axis;        /* [0] 0 = map +z, 1 = the particle's own body z, R * (0, 0, 1) */
  float height;         /* [0.0] base frame above the contact point, metres; finite, >= 0 */
  float probe_up;       /* [0.3] the step height the robot climbs; finite, >= 0 */
  float probe_down;     /* [1.0] how far below the contact point the surface may be; finite, >= 0 */
  float min_up_cos;     /* [0.7] faces with |n . a| below it are walls, not ground; in [0, 1] */
  uint32_t align;       /* [0] 0 = position only, 1 = also put body z on the face normal */
  uint32_t on_miss;     /* [0] 0 = leave a particle without ground as it is, 1 = likelihood {0, 0, max_n_meas} as the collision test writes it */
} rmclhip_surface_params;
/* what the last constrained call did: n_particles = n_snapped + n_missed + n_steep */
typedef struct { uint32_t n_particles, n_snapped, n_missed, n_steep; } rmclhip_surface_stats;

/* sensor_msgs/PointCloud2 layout of the fields this path reads (datatype: PointField FLOAT32 = 7, FLOAT64 = 8) and
 * the row / column sub-sampling of rmcl::FilterOptions2D (scan_operations.cpp:41-52) */
typedef struct {
  uint32_t width, height, point_step, row_step;
  uint32_t offset_x, offset_y, offset_z;
  uint32_t datatype;
} rmclhip_pointcloud2_layout;
typedef struct { uint32_t skip_begin, skip_end, increment; } rmclhip_filter1d;

/* rmcl::GladiatorResamplerConfig (GladiatorResamplerConfig.hpp:7-20), defaults GladiatorResamplerGPU.cpp:34-44 */
typedef struct {
  float min_noise_tx, min_noise_ty, min_noise_tz;        /* 0.03 0.03 0 */
  float min_noise_roll, min_noise_pitch, min_noise_yaw;  /* 0 0 0.01 */
  float likelihood_forget_per_meter;                     /* 0.3 */
  float likelihood_forget_per_radian;                    /* 0.2 */
  uint32_t trans_dist_metric; /* 0 = |t| (resampling.cu:179), 1 = |t|^2 (GladiatorResamplerCPU.cpp:156) */
} rmclhip_gladiator_config;
/* rmcl::SimpleLikelihoodStats (resampling.cuh:26-30) */
typedef struct { float sum, max; } rmclhip_likelihood_stats;
/* rmcl_msgs/ParticleStats as RmclNode::estimateStats fills it (rmcl_localization.cpp:642-731) */
typedef struct {
  rmclhip_transform pose;           /* rm::markley_mean of the poses, weights likelihood.mean / sum (:703-705) */
  double covariance[36];            /* rm::covariance around that mean (:716-718), row-major 6x6: x y z roll pitch yaw */
  double likelihood_mean, likelihood_sigma, likelihood_min, likelihood_max;   /* :664-689 */
  float trans_bb_min[3], trans_bb_max[3];
  uint32_t n_particles;             /* min(n_particles, max_induction_particles) */
  uint32_t reserved;
} rmclhip_pose_estimate;

typedef struct {
  uint32_t n_faces, n_vertices;
  uint32_t n_nodes;        /* BVH4 nodes (128 B each) */
  uint32_t n_tri_records;  /* 64 B each, leaf order; >= n_faces: a face that the builder's spatial splits reference from k leaves has k
                            * identical records (round 6; == n_faces for maps no spatial split touched) */
  uint32_t max_depth;      /* BVH4 depth */
  uint32_t stack_need;     /* worst-case traversal stack entries */
  uint64_t device_bytes;
  float bbox_min[3], bbox_max[3];
  /* round 5: stack_need <= 64 holds for EVERY mesh (no mesh is refused for its shape; rm::import_embree_map takes any Assimp mesh,
     micp_localization.cpp:187-195).  These two count how often the bound had to be enforced -- 0 on ordinary meshes: object-median
     splits forced by the height budget of the binary tree, and BVH4 nodes expanded tallest-child-first instead of largest-area-first */
  uint32_t height_fallbacks, guarded_nodes;
  /* round 6: spatial splits (SBVH) the builder took: nodes cut by a plane, a straddling triangle referenced from both sides with the box
   * of its part there.  0 on regular meshes (the object split is kept unless the spatial one is >= 10 % cheaper); CAD-like mixes of
   * huge and tiny triangles and slivers get them, within a budget of extra records (n_tri_records - n_faces). */
  uint32_t spatial_splits, reserved;
} rmclhip_map_info;

typedef struct rmclhip_ctx rmclhip_ctx;
typedef struct rmclhip_map rmclhip_map;
typedef struct rmclhip_rcc rmclhip_rcc;
typedef struct rmclhip_pf rmclhip_pf;
typedef struct rmclhip_resampler rmclhip_resampler;
typedef struct rmclhip_comm rmclhip_comm;              /* RCCL communicators of one process driving several devices */
typedef struct rmclhip_pf_sharded rmclhip_pf_sharded;  /* a particle cloud block-partitioned over those devices */
typedef struct rmclhip_rcc_sharded rmclhip_rcc_sharded; /* one correspondence operator per device: pose batches block-partitioned */
typedef struct rmclhip_field rmclhip_field;            /* the distance field of a map: a lattice of distances to the closest triangle */

/* ---- library ------------------------------------------------------------------ */
const char* rmclhip_last_error(void);
const char* rmclhip_version(void);

/* context = one device (+ default resources). device index as seen by HIP.  The context is reference counted:
 * every map / rcc / pf / resampler handle created from it holds a reference, rmclhip_ctx_destroy drops the
 * creator's, and the context is freed with its last holder -- destroy order does not matter. */
rmclhip_status rmclhip_ctx_create(int device, rmclhip_ctx** out);
void rmclhip_ctx_destroy(rmclhip_ctx* ctx);

/* How the SYNCHRONOUS calls that return a result through host-mapped memory (computeCrossStatistics, correct_once,
 * micp_correct_once) wait for it.  RMCLHIP_WAIT_SPIN (default): the calling thread polls a completion tag the last kernel
 * of the call writes (sequence number + checksum of the result, verified by the host) -- ~9 us less latency per call, one
 * busy host core while a call is in flight.  RMCLHIP_WAIT_BLOCK: hipStreamSynchronize -- the thread sleeps in the runtime.
 * The reference's node has ONE correction thread per node (micp_localization.cpp:300-302); integrators who cannot spare a
 * spinning core choose BLOCK.  Applies to every handle of the context, may be changed at any time.
 * Since round 4 the synchronous calls that return NOTHING through the host (find, find_cpc, pf_update, pf_motion_update,
 * pf_extract_weights, resampler_gladiator) wait the same way in SPIN mode: a one-thread launch behind the call's kernels stores
 * the tag (a 128x1024 find returns after 24.5 instead of 31.6 us); the call's results are complete when it returns either way. */
#define RMCLHIP_WAIT_SPIN 0
#define RMCLHIP_WAIT_BLOCK 1
rmclhip_status rmclhip_ctx_set_wait_mode(rmclhip_ctx* ctx, int mode);
rmclhip_status rmclhip_ctx_device_name(rmclhip_ctx* ctx, char* buf, size_t n);

/* ---- map ------------------------------------------------------------------------
 * replaces rm::import_embree_map / import_optix_map + scene commit
 * (micp_localization.cpp:187-195; PCDSensorUpdaterEmbree.cpp:143-174): copies the
 * indexed triangle mesh, builds the BVH on the host, uploads; immutable afterwards.
 * Ref-counted so it can live in an rm::MapMap-like registry under "<name>.hip". */
rmclhip_status rmclhip_map_create(rmclhip_ctx* ctx, const float* vertices_xyz, uint32_t n_vertices,
                                  const uint32_t* faces_ijk, uint32_t n_faces, rmclhip_map** out);
rmclhip_status rmclhip_map_retain(rmclhip_map* map);
void rmclhip_map_release(rmclhip_map* map);
rmclhip_status rmclhip_map_get_info(const rmclhip_map* map, rmclhip_map_info* out);

/* A whole scene: n_meshes indexed meshes, placed -- and possibly repeated -- by n_instances affine transforms.  This is what
 * rm::import_embree_map / import_optix_map make of an assimp scene (micp_localization.cpp:187-195: one mesh per aiMesh, one
 * instance per aiNode that references it).  The scene is flattened on the host into ONE world-space triangle soup and one
 * tree (an instance costs its triangles again; RMCL's maps are a few static meshes).  instances == NULL: every mesh once,
 * untransformed (n_instances is ignored).  transform: the first three rows of the row-major 4x4 node matrix (aiMatrix4x4's
 * own layout, a1..c4), p_map = A p_mesh + t, applied in float row by row.  Face ids the find / download calls return are
 * GLOBAL: instance i owns ids [first_face[i], first_face[i+1]), in the mesh's own face order. */
typedef struct {
  const float* vertices_xyz;
  const uint32_t* faces_ijk;
  uint32_t n_vertices, n_faces;
} rmclhip_mesh;
typedef struct {
  float transform[12];   /* rows of [A | t] */
  uint32_t mesh;         /* index into meshes[] */
  uint32_t reserved[3];
} rmclhip_instance;
rmclhip_status rmclhip_map_create_scene(rmclhip_ctx* ctx, const rmclhip_mesh* meshes, uint32_t n_meshes,
                                        const rmclhip_instance* instances, uint32_t n_instances, rmclhip_map** out);
/* the face-id offset table of a map: first_face_out gets n_instances + 1 entries (the last = n_faces); a map made by
 * rmclhip_map_create reports one instance.  first_face_out may be NULL to query n_instances. */
rmclhip_status rmclhip_map_scene_instances(const rmclhip_map* map, uint32_t* first_face_out, size_t capacity,
                                           uint32_t* n_instances);
/* global face id -> (instance, face index within that instance's mesh) */
rmclhip_status rmclhip_map_scene_locate(const rmclhip_map* map, uint32_t face_id, uint32_t* instance, uint32_t* local_face);
/* the flattening alone, host only (no device): what rmclhip_map_create_scene hands to the BVH builder.  Output pointers may
 * be NULL to query the sizes. */
rmclhip_status rmclhip_scene_flatten_host(const rmclhip_mesh* meshes, uint32_t n_meshes, const rmclhip_instance* instances,
                                          uint32_t n_instances, float* vertices_out, size_t vertices_cap_floats,
                                          uint32_t* faces_out, size_t faces_cap_dwords, uint32_t* first_face_out,
                                          size_t first_face_cap, uint32_t* n_vertices, uint32_t* n_faces);

/* Host-only BVH build (no device needed): fills caller buffers with the exact
 * arrays map_create uploads.  nodes: n_nodes*32 dwords, tris: n_tri_records*16 dwords.
 * Pass NULL buffers to query sizes via info.  Used by the CPU tests to check the
 * builder's invariants without a GPU. */
rmclhip_status rmclhip_bvh_build_host(const float* vertices_xyz, uint32_t n_vertices,
                                      const uint32_t* faces_ijk, uint32_t n_faces,
                                      rmclhip_map_info* info, uint32_t* nodes_out, size_t nodes_cap_dwords,
                                      uint32_t* tris_out, size_t tris_cap_dwords);
/* the 64-B quantised twins of the nodes (layout.h: Node4Q, 16 dwords each, same indices and child references as the
 * Node4 array of rmclhip_bvh_build_host): what the incoherent traversals (particle filter, pose batches) read */
rmclhip_status rmclhip_bvh_build_host_quantised(const float* vertices_xyz, uint32_t n_vertices, const uint32_t* faces_ijk,
                                                uint32_t n_faces, uint32_t* qnodes_out, size_t qnodes_capacity_dwords);
/* the frontier table of the map's tree (pf_tree = 0) or of the particle filter's (1) -- the <= 256 child references at depth 4 where
 * a scan's rays start, 8 dwords each {lo.xyz hi.x | hi.yz ref pad} -- and its 16 group boxes in the same format: group g = the union
 * of the stored boxes of table entries 16 g ... 16 g + 15, ref = how many entries it covers, the far point where it covers none.  A
 * wave tests the groups first and skips the blocks of the table whose groups lie outside its tile's pyramid.  Either buffer may be
 * null; *n_table / *n_groups receive the entry counts (n_groups is 16, or 0 for an empty table). */
rmclhip_status rmclhip_bvh_build_host_frontier(const float* vertices_xyz, uint32_t n_vertices, const uint32_t* faces_ijk,
                                               uint32_t n_faces, int pf_tree, uint32_t* table_out, size_t table_capacity_dwords,
                                               uint32_t* n_table, uint32_t* groups_out, size_t groups_capacity_dwords,
                                               uint32_t* n_groups);

/* the particle filter's own tree of the same map: the builder splits ONE BVH2 down to leaves of <= 2 triangles; the map's
 * tree (leaves <= 4, rmclhip_bvh_build_host) and this one are two cuts through it and share the leaf-ordered record
 * array.  nodes_out: Node4 (32 dwords each), qnodes_out: Node4Q (16 dwords each, what k_pf_update_* reads); either may be
 * null; info->n_nodes / max_depth / stack_need describe THIS tree.  Replaces nothing in the reference (Embree / OptiX
 * build their own acceleration structures, PCDSensorUpdaterEmbree.cpp:158, PCDSensorUpdaterOptix.cpp:123-154). */
rmclhip_status rmclhip_bvh_build_host_pf(const float* vertices_xyz, uint32_t n_vertices, const uint32_t* faces_ijk,
                                         uint32_t n_faces, rmclhip_map_info* info, uint32_t* nodes_out,
                                         size_t nodes_cap_dwords, uint32_t* qnodes_out, size_t qnodes_cap_dwords);

/* ---- ray-casting correspondences (MICP-L) ------------------------------------------
 * rmcl::RCCEmbreeSpherical / RCCEmbreeO1Dn / RCCOptixSpherical
 * (rmcl/include/rmcl/registration/RCCEmbree.hpp:18-83, RCCOptix.hpp:18-93) on top of
 * rmcl::Correspondences_<MemT> (Correspondences.hpp:16-88). */
rmclhip_status rmclhip_rcc_create(rmclhip_ctx* ctx, rmclhip_map* map, rmclhip_rcc** out);
void rmclhip_rcc_destroy(rmclhip_rcc* rcc);
/* Correspondences_::setTsb (Correspondences.hpp:31-34; RCCEmbree.cpp:15-19) */
rmclhip_status rmclhip_rcc_set_tsb(rmclhip_rcc* rcc, const rmclhip_transform* Tsb);
/* rm::ModelSetter<SphericalModel>::setModel (RCCEmbree.cpp:21-24) */
rmclhip_status rmclhip_rcc_set_model_spherical(rmclhip_rcc* rcc, const rmclhip_spherical_model* model);
/* rm::ModelSetter<O1DnModel>::setModel (RCCEmbree.cpp:84-87; fields conversions.cpp:74-94):
 * dirs_xyz is width*height*3 floats, row-major buffer id = vid*width + hid */
rmclhip_status rmclhip_rcc_set_model_o1dn(rmclhip_rcc* rcc, uint32_t width, uint32_t height,
                                          rmclhip_interval range, rmclhip_vec3 orig, const float* dirs_xyz);
/* rm::ModelSetter<PinholeModel>::setModel (RCCEmbreePinhole, RCCEmbree.cpp:39-68; f = {fx, fy}, c = {cx, cy}:
 * conversions.cpp:36-60): direction = normalize((hid-cx)/fx, (vid-cy)/fy, 1) mapped optical -> x-forward frame */
rmclhip_status rmclhip_rcc_set_model_pinhole(rmclhip_rcc* rcc, uint32_t width, uint32_t height,
                                             rmclhip_interval range, float fx, float fy, float cx, float cy);
/* rm::ModelSetter<OnDnModel>::setModel (RCCEmbreeOnDn, RCCEmbree.cpp:102-130; fields conversions.cpp:96-120):
 * one origin AND one direction per ray, width*height*3 floats each, buffer id = vid*width + hid */
rmclhip_status rmclhip_rcc_set_model_ondn(rmclhip_rcc* rcc, uint32_t width, uint32_t height,
                                          rmclhip_interval range, const float* origs_xyz, const float* dirs_xyz);
/* public members Correspondences_::params.max_dist / adaptive_max_dist_min
 * (written by the node: micp_localization.cpp:608-609) */
rmclhip_status rmclhip_rcc_set_params(rmclhip_rcc* rcc, float max_dist, float adaptive_max_dist_min);
/* Correspondences_::dataset {points, mask} (filled by MICPSphericalSensorCPU::unpackMessage,
 * MICPSphericalSensorCPU.cpp:181-233).  src_is_device != 0: pointers are device memory.
 * mask may be NULL (all valid). */
rmclhip_status rmclhip_rcc_set_dataset(rmclhip_rcc* rcc, const float* points_xyz, const uint8_t* mask,
                                       uint32_t n, int src_is_device);
/* Correspondences_::dataset kept in the CALLER's device memory (rmagine::PointCloud_<VRAM_HIP>: Correspondences.hpp:24,
 * written by `correspondences_->dataset.points = dataset_cpu_.points`, MICPSphericalSensorCUDA.cpp:231-232): the handle
 * borrows the pointers -- no copy -- until the next set_dataset* call; the memory must stay valid meanwhile.
 * mask_dev may be NULL (all valid). */
rmclhip_status rmclhip_rcc_set_dataset_view(rmclhip_rcc* rcc, const float* points_xyz_dev, const uint8_t* mask_dev, uint32_t n);
/* convenience mirror of unpackMessage: ranges -> dataset points = dir(vid,hid)*range (+orig for
 * O1Dn), mask = range in [range.min, range.max]; returns valid count */
rmclhip_status rmclhip_rcc_set_dataset_from_ranges(rmclhip_rcc* rcc, const float* ranges, uint32_t n,
                                                   uint32_t* n_valid_out);
/* RCC*::find(Tbm_est) (RCCEmbree.cpp:26-36, RCCOptix.cpp:28-43): grow-only model buffers,
 * simulate {points, normals, hits} (+ ranges, face ids) in the SENSOR frame. No-op on an empty model. */
rmclhip_status rmclhip_rcc_find(rmclhip_rcc* rcc, const rmclhip_transform* Tbm_est);
rmclhip_status rmclhip_rcc_find_async(rmclhip_rcc* rcc, const rmclhip_transform* Tbm_est);
rmclhip_status rmclhip_rcc_sync(rmclhip_rcc* rcc);
/* Wire-format input: the bytes of a sensor_msgs/PointCloud2 become the O1Dn sensor model AND the dataset in one
 * device pass -- estimateModelAndData (rmcl_ros/src/util/conversions.cpp:869-1002: range = |p|, dir = p / range,
 * non-finite -> 0) + filter (scan_operations.cpp:41-116; NULL = keep every row / column) +
 * MICPO1DnSensorCPU::unpackMessage (MICPO1DnSensorCPU.cpp:176-227: point = dir * range + orig,
 * mask = range within `range`).  Replaces set_model_o1dn + set_dataset for clouds; `data` may be a host or a
 * device pointer.  Returns the filtered image size and the number of valid measurements. */
rmclhip_status rmclhip_rcc_set_input_pointcloud2(rmclhip_rcc* rcc, const uint8_t* data, size_t nbytes,
                                                 const rmclhip_pointcloud2_layout* layout,
                                                 const rmclhip_filter1d* filter_height,
                                                 const rmclhip_filter1d* filter_width, rmclhip_interval range,
                                                 int src_is_device, uint32_t* out_width, uint32_t* out_height,
                                                 uint32_t* n_valid);
/* Wire-format input of the SPHERICAL model: the bytes of a (usually unorganised) sensor_msgs/PointCloud2 are binned into the
 * (phi, theta) grid of a spherical model on the device -- Pc2ToScanNode::convert (rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213),
 * empty cells as scan_operations.cpp:25-39.  Per point i in buffer order (i = row * width + col at row * row_step + col * point_step):
 *   1. x, y, z: FLOAT32, or FLOAT64 cast to float; skipped unless all three are finite (NaN and +-inf)
 *   2. ps = T_sensor_cloud * (x, y, z) (NULL: same frame)
 *   3. range_est = sqrtf((x*x + y*y) + z*z) of ps; theta_est = (float)atan2((double)y, (double)x);
 *      phi_est = (float)atan2((double)z, (double)range_est)  -- the reference's rule; it is atan(sin(elevation)), see TRUE_ELEVATION
 *   4. id = (int)(((est - min) / inc) + 0.5): the quotient in float, + 0.5 in double, truncated toward zero, compared in double with
 *      [0, size) (NaN rejects).  inc == 0 is accepted for size == 1 only: every point then has id 0 on that axis.  A negative inc is
 *      accepted as it is: ids count from min DOWNWARD (phi.min > 0 with phi.inc < 0: row 0 is the top row), nothing is refused
 *   5. a point inside the image with range_est inside [range.min, range.max] is a candidate of cell phi_id * W + theta_id; the
 *      candidate with the LARGEST i wins (the reference's sequential overwrite)
 *   6. ranges[cell] = the winner's range_est, or (float)((double)range.max + 1.0) for a cell nobody hit
 * The default repeats the reference statement for statement; each flag corrects one of its findings:
 *   TRUE_ELEVATION  phi_est = atan2(z, sqrt(x*x + y*y)): the inverse of the model's dir(vid, hid)
 *   FLOOR           id = floor(q + 0.5): truncation also takes q + 0.5 in (-1, 0) into cell 0
 *   WRAP_THETA      theta ids outside [0, W) are moved by one period when 2 pi / theta.inc is a whole number (within 1e-3): for
 *                   theta.min = -pi the column hid = 0 computes theta_est = +pi and is lost otherwise
 *   NEAREST         a cell keeps its SMALLEST range (ties: the smaller i) instead of its last point: independent of the buffer order
 * The winner is resolved with integer atomics on (i, range) keys: the same bits on every run.  stats (nullable): points in the
 * layout, with finite x / y / z, inside the image, inside the image and the range interval, and the number of cells that hold a point.
 * Unknown flag bits, a null layout / model / data with points, data shorter than its layout, a non-finite T, a zero increment with
 * size != 1, more than 2^31 points or cells: RMCLHIP_ERR_INVALID; a datatype other than 7 / 8: RMCLHIP_ERR_UNSUPPORTED.  An empty
 * cloud is no error: an all-empty image, zero counts. */
#define RMCLHIP_PC2SCAN_TRUE_ELEVATION 1u
#define RMCLHIP_PC2SCAN_FLOOR          2u
#define RMCLHIP_PC2SCAN_WRAP_THETA     4u
#define RMCLHIP_PC2SCAN_NEAREST        8u
typedef struct { uint32_t n_points, n_finite, n_in_image, n_in_range, n_cells_filled; } rmclhip_pc2scan_stats;
/* free function on a stream of the context's own (calls on one context serialise); data and ranges_out (theta.size * phi.size floats)
 * each in host or in device memory; synchronous */
rmclhip_status rmclhip_pointcloud2_to_scan(rmclhip_ctx* ctx, const uint8_t* data, size_t nbytes,
                                           const rmclhip_pointcloud2_layout* layout, int src_is_device,
                                           const rmclhip_transform* T_sensor_cloud, const rmclhip_spherical_model* model,
                                           uint32_t flags, float* ranges_out, int ranges_is_device, rmclhip_pc2scan_stats* stats);
/* On an operator with a spherical model (RMCLHIP_ERR_INVALID otherwise): the same image becomes the dataset, as
 * rmclhip_rcc_set_dataset_from_ranges makes it (MICPSphericalSensorCPU::unpackMessage, :181-233: points = dir(vid, hid) * range,
 * mask = range inside the model's interval) -- in the same pass, the image never leaves the device.  The MODEL is not touched:
 * W, H, the tile planes and a captured graph stay valid from scan to scan (unlike rmclhip_rcc_set_input_pointcloud2, which
 * rebuilds an O1Dn model per cloud).  Host bytes are staged in a grow-only buffer; image and per-cell scratch are grow-only members:
 * a repeated call allocates nothing.  ranges_dev_out (nullable): the image in device memory, borrowed, valid until the next
 * rmclhip_rcc_set_input_pointcloud2_scan call -- what rmclhip_rcc_segment accepts as device ranges.  stats->n_cells_filled is the
 * dataset's valid count (while range.max + 1 is representable above range.max). */
rmclhip_status rmclhip_rcc_set_input_pointcloud2_scan(rmclhip_rcc* rcc, const uint8_t* data, size_t nbytes,
                                                      const rmclhip_pointcloud2_layout* layout, int src_is_device,
                                                      const rmclhip_transform* T_sensor_cloud, uint32_t flags,
                                                      const float** ranges_dev_out, rmclhip_pc2scan_stats* stats);

/* ---- MOTION-COMPENSATED INPUT: a PointCloud2 taken while the sensor moved, every point from its own pose ----
 * A spinning LiDAR takes 50-100 ms per revolution; the drivers stamp every point.  The calls above treat a scan as taken from one
 * pose.  These take the cloud's per-point time field and the sensor's motion during the scan and cast every ray from the pose the
 * sensor had when it measured it: an OnDn model (one origin per ray) plus the dataset, in one device pass.
 *
 * Motion of a scan: K knots, 2 <= K <= 64.  times[k]: doubles, seconds, strictly increasing.  knots[k] = T_sref_s(t_k): the sensor
 * frame at t_k expressed in the sensor frame at the REFERENCE time -- the stamp the caller localises at; the knot at that time is the
 * identity.  (stamp of a knot is ignored.)
 * Time of a point: t = offset_s + scale * raw, in double; raw is the time field at byte `offset` of the record: PointField UINT32
 * (6: Ouster t, ns -> scale 1e-9), FLOAT32 (7: Velodyne time) or FLOAT64 (8); any other datatype: RMCLHIP_ERR_UNSUPPORTED.
 * Pose of a point:
 *   k = the largest index with times[k] <= t, limited to [0, K - 2]
 *   s = (float)((t - times[k]) / (times[k+1] - times[k])), the quotient in double; s < 0 or s > 1 is clamped to that end -- the point
 *       takes the end knot and is counted in n_time_clamped
 *   float from here on, every step one IEEE operation:  a = 1.0f - s;  q' = -q_{k+1} if ((qx qx' + qy qy') + qz qz') + qw qw' < 0
 *   (the shorter arc), else q_{k+1};  q = a * q_k + s * q' per component, each divided by sqrtf(((x*x + y*y) + z*z) + w*w);
 *   tr = a * t_k + s * t_{k+1} per component.
 *   This is nlerp, not slerp, on purpose: no transcendental on the device, so a float32 restatement on the host (tests/deskew_ref.py)
 *   reproduces the bytes.  Over a segment that turns by theta, nlerp stays on slerp's arc and is off along it by at most
 *   theta^3 / (144 sqrt 3) ~ theta^3 / 249 to leading order in theta (the next term adds theta^2 / 80 of that; attained at s = 0.21
 *   and 0.79, zero at both ends and in the middle): 1.1e-4 rad for a 0.3 rad scan
 *   in ONE segment, 2.6e-8 rad -- below 2^-24, the resolution of a float quaternion -- in 16.  The caller makes the knots that
 *   dense; rmclhip_scan_motion_from_base_poses_host subdivides by true slerp in double.
 *   A non-finite t takes knots[0], is counted in n_time_nonfinite (not in n_time_clamped) and has mask 0.
 * Outputs per point, i = ti * out_w + tj over the rows / columns the filters keep (as rmclhip_rcc_set_input_pointcloud2):
 *   x, y, z as there (FLOAT64 cast to float); one of them non-finite: range = 0, dir_local = 0; else
 *   range = sqrtf((x*x + y*y) + z*z), dir_local = (x, y, z) / range
 *   orig_i = tr;  dir_i = q * dir_local (the Hamilton product q (d, 0) q^-1 of rmclhip_transform);  point_i = dir_i * range + orig_i
 *   mask_i = range within `range` and t finite
 * With identity knots every output is, bit for bit, what rmclhip_rcc_set_input_pointcloud2 writes for the same bytes, all origins
 * +0 (but for the sign of a coordinate that is -0 in the cloud).
 * stats (nullable): n_points = out_w * out_h, n_finite (x, y, z finite), n_valid (mask 1), n_time_clamped, n_time_nonfinite.
 * RMCLHIP_ERR_INVALID, before anything is launched, outputs and the operator's state untouched: a null layout; null data / time /
 * motion / knots / times with points to read; data shorter than the last byte a kept point's x / y / z / time field reaches;
 * K outside [2, 64]; non-finite or non-increasing knot times; a non-finite knot, or a quaternion whose norm is off 1 by more than
 * 1e-3; a non-finite scale or offset_s; bad filters; more than 2^31 points.  An empty cloud is no error. */
typedef struct { uint32_t offset, datatype; double scale, offset_s; } rmclhip_pointcloud2_time;
typedef struct { const rmclhip_transform* knots; const double* times; uint32_t n_knots; } rmclhip_scan_motion;
typedef struct { uint32_t n_points, n_finite, n_valid, n_time_clamped, n_time_nonfinite; } rmclhip_deskew_stats;
/* The operator form: the operator becomes OnDn (out_w x out_h rays, as rmclhip_rcc_set_model_ondn leaves it: tuned kinds reset, no
 * frontier start) with the dataset set, as set_model_ondn + set_dataset of the arrays above would leave it -- without the host loop
 * and the two uploads.  `data` may be a host or a device pointer; buffers are grow-only, a repeated call allocates nothing. */
rmclhip_status rmclhip_rcc_set_input_pointcloud2_deskewed(rmclhip_rcc* rcc, const uint8_t* data, size_t nbytes,
                                                          const rmclhip_pointcloud2_layout* layout,
                                                          const rmclhip_pointcloud2_time* time,
                                                          const rmclhip_filter1d* filter_height, const rmclhip_filter1d* filter_width,
                                                          rmclhip_interval range, int src_is_device, const rmclhip_scan_motion* motion,
                                                          uint32_t* out_width, uint32_t* out_height, rmclhip_deskew_stats* stats);
/* The cloud form, a free function on the context's PointCloud2 stream (calls on one context serialise; synchronous): every point of
 * the layout (no filters) as one 12-byte xyz float record in points_out_dev (device memory, width * height records), in the sensor
 * frame of the reference time; NaN where the mask would be 0.  The records are byte-equal to the operator form's points.  They are a
 * valid src_is_device input of rmclhip_rcc_set_input_pointcloud2_scan (point_step 12, offsets 0 / 4 / 8, FLOAT32): the spherical fast
 * path -- points moved, rays cast from the reference pose.  That NEGLECTS THE PARALLAX of the ray origins (up to the distance the
 * sensor moved, seen from the surface's range); the operator form does not.  They are also valid for rmclhip_rcc_set_dataset_view +
 * rmclhip_rcc_find_cpc: closest-point correspondences need no rays, so that path is exact. */
rmclhip_status rmclhip_pointcloud2_deskew(rmclhip_ctx* ctx, const uint8_t* data, size_t nbytes,
                                          const rmclhip_pointcloud2_layout* layout, const rmclhip_pointcloud2_time* time,
                                          int src_is_device, const rmclhip_scan_motion* motion, rmclhip_interval range,
                                          float* points_out_dev, rmclhip_deskew_stats* stats);
/* HOST function, in double: the motion of a scan from n >= 2 base poses T_x_b[i] (base in any fixed frame x: odometry) at strictly
 * increasing times[i].  The base pose at t_ref (within [times[0], times[n-1]]) is interpolated by slerp + lerp; knot k is
 * ~Tsb * ~T_x_b(t_ref) * T_x_b(t_k) * Tsb.  Every segment gets subdivide - 1 >= 0 further knots by slerp + lerp, evenly in time:
 * (n - 1) * subdivide + 1 knots in all, written to knots_out / times_out (capacity entries each); *n_out: their number.
 * RMCLHIP_ERR_INVALID: null arguments, n < 2, subdivide == 0, non-finite or non-increasing times, t_ref outside them, a non-finite
 * pose or a zero quaternion, a result beyond capacity or beyond 64 knots (nothing is written then). */
rmclhip_status rmclhip_scan_motion_from_base_poses_host(const rmclhip_transform* Tsb, const rmclhip_transform* T_x_b,
                                                        const double* times, uint32_t n, double t_ref, uint32_t subdivide,
                                                        rmclhip_transform* knots_out, double* times_out, uint32_t capacity,
                                                        uint32_t* n_out);
/* The operator's inputs in device memory, borrowed -- valid until the next set_model_* / set_dataset* / set_input_* call of this
 * operator: the sensor model's table (spherical: cos phi | sin phi | cos theta | sin theta; O1Dn: width * height directions; OnDn:
 * width * height origins, then as many directions; pinhole or no model: NULL), the model's size, the dataset's points and mask
 * (NULL: none) and its size -- what a caller reads the compensated points of rmclhip_rcc_set_input_pointcloud2_deskewed from.
 * Every out pointer is nullable.  Waits for the operator's stream. */
rmclhip_status rmclhip_rcc_input_views(rmclhip_rcc* rcc, const float** model_table_dev, uint32_t* width, uint32_t* height,
                                       const float** dataset_points_dev, const uint8_t** dataset_mask_dev, uint32_t* n_dataset);
/* rmcl::CPCEmbree::find (rmcl/src/rmcl/registration/CPCEmbree.cpp:18-44), closest-point correspondences (`type: CP`):
 * for every dataset point Pm = Tsm * d_i the nearest surface point of the map; model buffers (sized like the
 * dataset) receive hits = (distance <= params.max_dist), points = Tms * p_closest, normals = Tms.R * n_face
 * (+ ranges = distance, face ids).  computeCrossStatistics then works unchanged. */
rmclhip_status rmclhip_rcc_find_cpc(rmclhip_rcc* rcc, const rmclhip_transform* Tbm_est);
/* Tracking (default on): the operator remembers which triangle every dataset point was closest to and starts the next
 * find_cpc of the SAME dataset with that triangle's distance as the search bound.  The triangle is a real candidate, so the
 * answer -- min distance, then min face id -- is the same bit for bit; what changes is the number of leaves a query visits
 * when the pose moved little between calls (an ICP loop).  A new dataset, or on = 0, starts cold. */
rmclhip_status rmclhip_rcc_set_cpc_tracking(rmclhip_rcc* rcc, int on);
/* Bounded search (default off = the reference's semantics, CPCEmbree.cpp:36-41: the global closest point of EVERY dataset point,
 * hits = (d <= params.max_dist)).  On: nothing farther than max_dist is looked for.  hits, and every output of a point that
 * hits, are unchanged bit for bit; a point with no surface within max_dist gets hits = 0 and NaN point / normal / distance,
 * face id 0xFFFFFFFF -- it is gated out of every statistic either way.  A first (cold) find then costs about what a tracked one
 * does; the two options combine. */
rmclhip_status rmclhip_rcc_set_cpc_bounded(rmclhip_rcc* rcc, int on);
/* The map's near grid (default on): ~2 M cubic cells over the map's box, each holding the triangle closest to its centre, built on the
 * first closest-point query of any operator of the map (one launch, a few ms, 4 B per cell).  A point without a tracking seed --
 * every point of a COLD query: first scan, new dataset, tracking off -- starts from the record of its cell: an actual candidate,
 * hence a bound within about a cell of the answer, so the cold query prunes like a tracked one (CPCEmbree.cpp:18-44 has no such
 * state: Embree's rtcPointQuery starts unbounded every time).  Results do not depend on it.  on = 0: A/B. */
rmclhip_status rmclhip_rcc_set_cpc_grid(rmclhip_rcc* rcc, int on);
/* Correspondences{CPU,CUDA}::computeCrossStatistics (CorrespondencesCPU.cpp:10-39):
 * max_dist' = max_dist (1-p) + adaptive_max_dist_min p; rm::statistics_p2l(T_snew_sold, ...)
 * Round 4: answered on the host from the moments of the current find's correspondences when a published set covers the call
 * (rmclhip_ccs_info below), by a streaming reduction otherwise -- same result.  CONTRACT that makes this sound: the dataset's
 * CONTENTS do not change between a find and the computeCrossStatistics calls that follow it unless one of the rmclhip_rcc_set_dataset*
 * calls announces it (they drop the set); the reference holds data_correction_mutex_ over both (micp_localization.cpp:868,968).
 * For the same reason rmclhip_rcc_find[_async] may READ the dataset (a find that was followed by such calls last time forms the
 * moments in its epilogue): a view handed over with rmclhip_rcc_set_dataset_view must stay valid until it is replaced. */
rmclhip_status rmclhip_rcc_compute_cross_statistics(rmclhip_rcc* rcc, const rmclhip_transform* T_snew_sold,
                                                    double convergence_progress,
                                                    rmclhip_cross_statistics* out);
/* modelView() read-back (Correspondences.hpp:47-55) + ranges / face ids. Any pointer may be NULL.
 * Sizes: n = model size of the last find. */
rmclhip_status rmclhip_rcc_download(rmclhip_rcc* rcc, uint8_t* hits, float* ranges, float* points_xyz,
                                    float* normals_xyz, uint32_t* face_ids);
/* borrowed device views of the model buffers (valid until the next find that grows them) */
rmclhip_status rmclhip_rcc_device_views(rmclhip_rcc* rcc, const uint8_t** hits_dev, const float** ranges_dev,
                                        const float** points_dev, const float** normals_dev,
                                        const uint32_t** face_ids_dev, uint32_t* n);
/* MICPLocalizationNode::correctOnce inner loop for ONE sensor, entirely on the device
 * (micp_localization.cpp:900-964 with MICPSensor.hpp:146-184): find(Tom*Tbo) once, then n_iter x
 * { T_bnew_bold = ~Tbo T_onew_oold Tbo; T_snew_sold = ~Tsb T_bnew_bold Tsb; reduce; Tsb*, Tbo*;
 *   umeyama; T_onew_oold *= T_inner }.  Outputs T_onew_oold and the last merged statistics (odom frame). */
rmclhip_status rmclhip_rcc_correct_once(rmclhip_rcc* rcc, const rmclhip_transform* Tom,
                                        const rmclhip_transform* Tbo, uint32_t n_iter,
                                        double convergence_progress, int refind_each_iteration,
                                        rmclhip_transform* T_onew_oold_out,
                                        rmclhip_cross_statistics* stats_o_out);
/* MICPLocalizationNode::correctOnce inner loop for N <= 8 sensors of one device (micp_localization.cpp:900-964): one find per
 * sensor at Tbm = Tom * Tbo[s], then n_iter x { per sensor statistics at T_snew_sold (MICPSensor.hpp:178) in its own frame,
 * Cs_o = Tbo * (Tsb * stats_s), Cmerged_o += Cs_o, Cmerged_weighted_o += Cs_o with n_meas *= merge_weight_multiplier[s]
 * (truncating, :934), T_onew_oold *= umeyama(Cmerged_weighted_o) } -- all on the device, one synchronisation at the end.
 * merge_weight_multiplier may be NULL (all 1); every weight must be finite and >= 0 (RMCLHIP_ERR_INVALID names the sensor otherwise:
 * the truncating conversion of a negative or non-finite product is undefined and differs between host and device).  A product
 * n_meas * weight of 2^32 or more is not checked and is the caller's to avoid.
 * merged_out: the UNWEIGHTED statistics of the last iteration (:1010-1011).
 * Every sensor's find (and moment pass) is enqueued on that sensor's OWN stream, so the scans run concurrently; the loop runs on
 * sensor 0's stream behind all of them (an in-kernel flag per sensor; stream events in the per-iteration fallback).  When the call
 * returns, all of it is complete and every sensor's model buffers hold its scan at Tom * Tbo[s]. */
rmclhip_status rmclhip_micp_correct_once(rmclhip_rcc* const* sensors, uint32_t n_sensors, const rmclhip_transform* Tom,
                                         const rmclhip_transform* Tbo, const double* merge_weight_multiplier, uint32_t n_iter,
                                         double convergence_progress, rmclhip_transform* T_onew_oold_out,
                                         rmclhip_cross_statistics* merged_out);
/* stale v1 SphereCorrector API (lidar_corrector_embree_benchmark.cpp:86-133): nposes hypotheses share
 * the dataset; one raycast + reduction + Umeyama per pose; Tdelta_out[i] such that
 * T_new[i] = Tbm[i] * Tdelta_out[i]. */
rmclhip_status rmclhip_rcc_correct_batch(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, uint32_t nposes,
                                         rmclhip_transform* Tdelta_out, rmclhip_cross_statistics* stats_out);

/* ---- pose batches over several devices (north_star: "pose-corrections/s at 1/2/4/8 GPUs"; SURVEY 8(e): MICP pose batches shard
 * by pose with NO exchange) -------------------------------------------------------------------------------------------------
 * One process, one operator replica per entry of `devices` (NULL: devices 0 .. ndev-1) over ONE host BVH build.  No collective is
 * involved, hence no RCCL communicator; an entry may repeat a device (two replicas on one GPU: of use to tests and to fill a GPU
 * that a single stream of small batches leaves idle).  Configure every replica through its borrowed handle with the ordinary
 * setters (rmclhip_rcc_set_tsb / _set_model_* / _set_params / _set_dataset*): the corrector does not care whether they agree.
 * rmclhip_rcc_sharded_correct_batch = rmclhip_rcc_correct_batch (the v1 SphereCorrector::correct shape,
 * lidar_corrector_optix_benchmark.cpp:86-133) with poses [lo, hi) = rmclhip_shard_bounds(nposes, rank, ndev) on replica `rank`:
 * every replica's chain is enqueued before any is waited for, results arrive in pose order, bit-identical to the unsharded call
 * (a pose's result does not depend on its neighbours in the batch). */
rmclhip_status rmclhip_rcc_sharded_create(const int* devices, uint32_t ndev, const float* vertices_xyz, uint32_t n_vertices,
                                          const uint32_t* faces_ijk, uint32_t n_faces, rmclhip_rcc_sharded** out);
void rmclhip_rcc_sharded_destroy(rmclhip_rcc_sharded* h);
uint32_t rmclhip_rcc_sharded_size(const rmclhip_rcc_sharded* h);
rmclhip_status rmclhip_rcc_sharded_replica(rmclhip_rcc_sharded* h, uint32_t rank, rmclhip_rcc** rcc_borrowed);
rmclhip_status rmclhip_rcc_sharded_correct_batch(rmclhip_rcc_sharded* h, const rmclhip_transform* Tbm, uint32_t nposes,
                                                 rmclhip_transform* Tdelta_out, rmclhip_cross_statistics* stats_out);

/* kernel variant selection: bits 0..3 (+ bit 13 = 16 more, bit 14 = 32 more) traversal kind.  15 = automatic, the
 * default: four lanes per ray up to 57344 rays in flight (kind 2); above that one lane per ray STARTING AT THE MAP'S FRONTIER (the
 * wave culls the <= 256 references of BFS depth 4 against its tile's pyramid and every ray tests the few survivors: the top levels of
 * the descent cost one cooperative pass) -- kind 23 on the full-precision nodes up to 262144 rays, kind 24 on the 64-B quantised
 * nodes of the particle filter's tree (leaves <= 2 triangles) above (large scans, pose batches).  librmclhip.so builds those three plus
 * 0 = wave packet and 32 (round 6) = the wave keeps descending COOPERATIVELY below the frontier: lane l tests entry (l & 15) of the
 * 16-wide twin of surviving node (l >> 4) against the tile's pyramid (two tree levels per round trip and wave instead of one round
 * trip per node visit and ray), then every ray marks the final leaves whose box it enters in a 64-bit mask and tests just those -- no
 * ordered hand-over, no stack.  29 % faster than 23 on the open benchmark map (C2 sphere-100k 17.2 -> 12.2 us, sphere-1M 22.3 -> 19.6),
 * slower on rooms whose grazing tiles see long strips of the map (room-100k 25.4 -> 30.8 us): the rule does not select it,
 * rmclhip_rcc_autotune measures it on the caller's map.  Every other kind (31 = round 6's first form of 32 with the sorted
 * hand-over among them) is a measured-and-rejected or superseded experiment that lives in librmclhip_lab.so (include/rmclhip_lab.h lists
 * them) and is accepted here only while that library is loaded (RMCLHIP_ERR_UNSUPPORTED otherwise),
 * bits 4..7 = 1 + log2(tile width) of the wave's scan-image tile (0 = automatic: 16 wide x 4 tall, 8x8 for the wave packet),
 * bit 9 = enqueue the per-iteration MICP loop directly instead of replaying it from a hipGraph (A/B).  Bits 8 and 10..12 (a
 * fused last-block reduction tail, reduce + solve launches, a persistent grid-barrier loop: MICP loop forms measured slower)
 * are retired: RMCLHIP_ERR_INVALID */
rmclhip_status rmclhip_rcc_set_variant(rmclhip_rcc* rcc, int variant);
/* Moment form of the schedule-(R) loop of rmclhip_rcc_correct_once (refind_each_iteration = 0; micp_localization.cpp:900-964
 * iterates statistics_p2l + umeyama over FIXED correspondences): the gate |dist| < max_dist is the only part of the 16 raw
 * sums that is not a polynomial in the pre-transform, so correspondences whose gate decision cannot change while the
 * pre-transform stays within bounds learnt from the previous corrections are summarised ONCE as 82 moments, the few others
 * are re-evaluated every iteration, and all iterations run in one single-workgroup launch.  When a pre-transform leaves the
 * bounds, or too many correspondences are undecided, the library falls back to one streaming launch per iteration: the
 * result never depends on the bounds (both forms agree to f64 summation order).  mode 0 = never; 1 = automatic (default): TWO plain
 * launches -- the find (per-ray kind 23 or quad kind 2: every single scan the rule serves) forms the moments in its epilogue, a
 * 10 x 10 product of factor vectors per correspondence through f64 MFMA; a fold launch sums the per-workgroup rows and publishes
 * {82 moments, the undecided correspondences (<= 1024)} to the host -- and the ITERATIONS RUN ON THE HOST (~0.5 us each; the same
 * published set then also answers rmclhip_rcc_compute_cross_statistics without a launch, see rmclhip_ccs_info); more than 1024
 * undecided: the device loop of mode 4 on the same rows.  3 = device loop, three plain launches (A/B: the moments always in a pass
 * of their own); 4 = device loop behind a find with the moment epilogue (round 3's default, A/B: one lane of the GPU solves every
 * iteration).  2 (the device loop replayed from a hipGraph, measured slower than direct launches) is retired: RMCLHIP_ERR_INVALID. */
typedef struct {
  uint32_t attempts, done, cap_exits, overflows;   /* outcomes since the operator was created */
  uint32_t last_code;                              /* 0 done, 1 pre-transform left the bounds, 2 too many undecided: > 1024 leaves the host form for the device loop, > 4096 the moment form altogether */
  uint32_t last_uncertain;                         /* undecided correspondences of the last attempt */
  float last_rho, last_tau;                        /* largest |2 sin(theta/2)| and |t| of its pre-transforms */
  float rho_cap, tau_cap;                          /* bounds the next attempt will use */
  uint32_t last_setup_clocks, last_loop_clocks;    /* diagnostics: shader clocks the single-workgroup launch spent before /
                                                    * in its iterations (last completed attempt; 0 when the host ran them) */
  uint32_t host_loops;                             /* attempts whose iterations ran on the host (mode 1) */
} rmclhip_micp_fast_info;
rmclhip_status rmclhip_rcc_set_micp_fast(rmclhip_rcc* rcc, int mode);
/* How rmclhip_rcc_compute_cross_statistics was served since the operator was created.  With the moment form on (mode != 0) a call is
 * answered ON THE HOST from the 82 moments + the undecided correspondences of the current find whenever a published set covers its
 * (pre-transform, max_dist'): no launch, no wait (micp_localization.cpp:915-964 calls it once per sensor and iteration on fixed
 * correspondences).  The set comes from the find itself when the previous find was followed by such calls (`speculative_finds`:
 * moment epilogue + publish, classified for max_dist' within +-8 % of the last one), else from ONE moment pass the first call
 * after a find pays (`passes`); everything else takes the streaming reduction (calls - from_moments). */
typedef struct {
  uint32_t calls;              /* computeCrossStatistics calls that were eligible (moment form on) */
  uint32_t from_moments;       /* ... answered on the host without a launch */
  uint32_t passes;             /* moment passes run by a call (no covering set yet) */
  uint32_t speculative_finds;  /* finds that formed the moments in their epilogue */
} rmclhip_ccs_info;
rmclhip_status rmclhip_rcc_ccs_info(const rmclhip_rcc* rcc, rmclhip_ccs_info* out);
/* The host half of the moment form on its own (no device): classifies the n correspondences (D = dataset point, I = model point,
 * N = model normal, valid nullable) for every max_dist' in [gate_lo, gate_hi] and every pre-transform within (rho_cap = |2 sin
 * theta/2|, tau_cap = |t|), accumulates the 82 moments of the certainly-gated-in ones, keeps the undecided ones (<= 1024 for the host, <= 4096 for the device loop), and
 * evaluates rm::statistics_p2l(Tpre, ..., max_dist) from them.  *covered = 0 (and Identity statistics) when (Tpre, max_dist) lies
 * outside what the set was formed for or more than 1024 correspondences are undecided: the library then uses the streaming
 * reduction.  What the device publishes per find is this set; the entry point exists so that the arithmetic can be checked
 * against the reference's per-element loop (MICPSensorCPU.cpp:70-84) without a GPU. */
rmclhip_status rmclhip_host_moment_statistics(const float* dataset_points, const float* model_points, const float* model_normals,
                                              const uint8_t* valid, uint32_t n, float gate_lo, float gate_hi, float rho_cap,
                                              float tau_cap, const rmclhip_transform* Tpre, float max_dist,
                                              rmclhip_cross_statistics* out, uint32_t* n_undecided, int* covered);
rmclhip_status rmclhip_rcc_micp_fast_info(const rmclhip_rcc* rcc, rmclhip_micp_fast_info* out);
/* the traversal (bits 0..3 above, never 15) a find of `nposes` scans of the current model would launch */
rmclhip_status rmclhip_rcc_find_variant(const rmclhip_rcc* rcc, uint32_t nposes, int* variant_out);
/* Measurement instead of brackets: the automatic rule above was tuned on two synthetic maps; which traversal is fastest for a
 * single scan depends on the map (open / occluded), the model's size and shape, and where the sensor is.  This call times the
 * product's single-scan kinds (2, 23, 24 -- the latter two with and without the frontier start -- and 32 with a short and a long list) on THIS operator's map and model at
 * the given pose (40 short launches each, HIP events), then the winner's tile shape (4, 8, 16 or 32 rays wide), then which workgroup
 * computes which tile (as the hardware deals workgroups over the XCDs -- the default --, an eighth of the image per XCD, or a CU's two
 * workgroups from the image's two halves), and makes the fastest combination the automatic choice for single scans until the model
 * or the tiling changes (~10 ms in all).  Results do not
 * depend on the kind (bit-identical); batches keep the rule.  Opt-in: never run behind the caller's back.
 * chosen_kind / kernel_ms may be NULL. */
rmclhip_status rmclhip_rcc_autotune(rmclhip_rcc* rcc, const rmclhip_transform* Tbm_est, int* chosen_kind, float* kernel_ms);
/* the same for pose batches (find_batch / correct_batch) of about nposes scans: kinds 23 / 24, each with and without the frontier
 * start (on an occluded map the per-wave culling can cost a batch more than the top levels it skips).  Both calls report the
 * choice as 2 / 23 / 24 / 32 or -- frontier start off -- as 19 / 22, round 2's numbers for the same traversals. */
rmclhip_status rmclhip_rcc_autotune_batch(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, uint32_t nposes, int* chosen_kind,
                                          float* kernel_ms);
/* rm::Simulator::simulate(Memory<Transform>, Bundle&) (batch form, lidar_corrector_embree_benchmark.cpp:117):
 * one launch for nposes x H x W rays; model buffers become pose-major [pose][vid][hid]. */
rmclhip_status rmclhip_rcc_find_batch(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, uint32_t nposes);

/* ---- the rmagine-level Simulator interface ---------------------------------------------------------------
 * The reference's RCC classes ARE simulators: `class RCCEmbreeSpherical : public CorrespondencesCPU, public
 * rmagine::ModelSetter<SphericalModel>, protected rmagine::SphereSimulatorEmbree` (rmcl/include/rmcl/registration/RCCEmbree.hpp:18-22),
 * find() is `simulate(Tbm_est, model_buffers_)` (RCCEmbree.cpp:35), and the simulators are also used on their own
 * (rmcl_ros/src/nodes/filter/scan_map_segmentation_embree.cpp:38-39,76-87; lidar_corrector_embree_benchmark.cpp:117).  Here the
 * rmclhip_rcc handle is that simulator: rmclhip_rcc_set_tsb / rmclhip_rcc_set_model_* are Simulator::setTsb / ::setModel, and
 * rmclhip_rcc_simulate is Simulator::simulate(const Transform&, BundleT&) / simulate(Memory<Transform>&, BundleT&).
 *
 * Bundle attribute selection.  rmagine's simulate<Bundle<Ranges, Normals>> writes only the attributes the bundle names
 * (scan_map_segmentation_embree.cpp:80-87); MICP's own bundle is {Points, Normals, Hits} = 25 B/ray (Correspondences.hpp:81-85).
 * An attribute is selected by a bit; the kernel skips the stores of the others. */
#define RMCLHIP_OUT_HITS 1u      /* rmagine::Hits     uint8  per ray */
#define RMCLHIP_OUT_RANGES 2u    /* rmagine::Ranges   float  per ray (miss: range.max + 1) */
#define RMCLHIP_OUT_POINTS 4u    /* rmagine::Points   3 floats, sensor frame (miss: NaN) */
#define RMCLHIP_OUT_NORMALS 8u   /* rmagine::Normals  3 floats, sensor frame, facing the ray (miss: NaN) */
#define RMCLHIP_OUT_FACE_IDS 16u /* rmagine::FaceIds  uint32 (miss: 0xFFFFFFFF) */
#define RMCLHIP_OUT_ALL 31u
#define RMCLHIP_OUT_MICP (RMCLHIP_OUT_HITS | RMCLHIP_OUT_POINTS | RMCLHIP_OUT_NORMALS) /* Correspondences_::model_buffers_ */
/* Which of the operator's OWN model buffers find / find_batch write (default RMCLHIP_OUT_ALL).  A deselected buffer is not written --
 * it keeps what the last find that selected it left there (nothing, if none did: download / device_views of it then fail / return
 * NULL).  computeCrossStatistics and the corrections read {hits, points, normals}: they fail with RMCLHIP_ERR_INVALID while one of
 * those is deselected.  mask == 0 or bits beyond RMCLHIP_OUT_ALL: RMCLHIP_ERR_INVALID. */
rmclhip_status rmclhip_rcc_set_outputs(rmclhip_rcc* rcc, uint32_t mask);
rmclhip_status rmclhip_rcc_get_outputs(const rmclhip_rcc* rcc, uint32_t* mask);
/* a rmagine Bundle over CALLER-owned device memory: one nullable pointer per attribute (NULL = the bundle does not carry it);
 * every non-null buffer holds nposes * width * height elements, index pose * W * H + vid * W + hid */
typedef struct {
  uint8_t* hits_dev;
  float* ranges_dev;
  float* points_xyz_dev;
  float* normals_xyz_dev;
  uint32_t* face_ids_dev;
} rmclhip_bundle_views;
/* rm::Simulator::simulate(const Transform& Tbm, BundleT& res) (nposes == 1; scan_map_segmentation_embree.cpp:87) and its batch form
 * simulate(const Memory<Transform>& Tbm, BundleT& res) (lidar_corrector_embree_benchmark.cpp:117, _optix_benchmark.cpp:119 -- there the
 * poses are device memory: Tbm_is_device != 0).  One launch for nposes x H x W rays with Tsm = Tbm[i] * Tsb, results in the sensor
 * frame into the caller's bundle.  The operator's own model buffers, its dataset and whatever computeCrossStatistics has cached of them
 * are NOT touched.  No-op on an empty model or nposes == 0.  The _async form returns once the launch is enqueued on the handle's stream
 * (rmclhip_rcc_sync waits); Tbm is copied before it returns. */
rmclhip_status rmclhip_rcc_simulate(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, uint32_t nposes, int Tbm_is_device,
                                    const rmclhip_bundle_views* out);
rmclhip_status rmclhip_rcc_simulate_async(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, uint32_t nposes, int Tbm_is_device,
                                          const rmclhip_bundle_views* out);
/* ---- map segmentation ------------------------------------------------------------------------------------------------------------
 * The per-scan body of ScanMapSegmentationEmbreeNode / O1DnMapSegmentationEmbreeNode (rmcl_ros/src/nodes/filter/
 * scan_map_segmentation_embree.cpp:76-185, o1dn_map_segmentation_embree.cpp; parameters map_segmentation.cpp:25-41) in one call: simulate
 * Bundle<Ranges, Normals> at Tsm = Tbm * Tsb, compare every simulated range with the measured one, and leave two clouds in BUFFER ORDER
 * (vid-major, the order the reference's loops push them in).  With inside(r) = range.min <= r && r <= range.max (NaN is outside; a
 * simulated miss is range.max + 1) for ray bid = vid * W + hid:
 *   both inside:  pint_s = dir * r_sim (NO origin, as the reference writes it), n = normalize(normal_sim),
 *                 plane_distance = |(preal_s - pint_s) . n| with preal_s = dir * r_real + orig;
 *                 r_real <  r_sim: plane_distance > min_dist_outlier_scan ? outlier_scan gets preal_s : inlier
 *                 r_real >= r_sim: plane_distance > min_dist_outlier_map  ? outlier_map  gets pint_s  : inlier
 *   real only:    outlier_scan gets preal_s
 *   sim only:     outlier_map gets dir * r_sim + orig
 *   neither:      nothing
 * Labels: one uint8 per ray, 0 none, 1 inlier, 2 outlier_scan, 3 outlier_map.  A cloud is packed xyz float32 (point_step 12: the `data`
 * of a PointCloud2 with the reference's SegmentationPoint fields).  RMCLHIP_SEG_PINT_WITH_ORIGIN adds the origin to pint_s in the
 * both-inside branch too (plane distance and emitted point): it only matters for O1Dn / OnDn models with an offset origin. */
#define RMCLHIP_SEG_PINT_WITH_ORIGIN 1u
typedef struct {
  float min_dist_outlier_scan, min_dist_outlier_map; /* metres, >= 0 (the reference's defaults: 0.15); compared with a strict > */
  uint32_t flags;                                    /* RMCLHIP_SEG_* */
} rmclhip_segmentation_params;
typedef struct {                  /* caller-owned device memory, every pointer nullable */
  uint8_t* labels_dev;            /* W*H */
  float* outlier_scan_xyz_dev;    /* capacity W*H points */
  float* outlier_map_xyz_dev;     /* capacity W*H points */
  uint32_t* counts_dev;           /* [2] = {n_outlier_scan, n_outlier_map}, for consumers that stay on the stream */
} rmclhip_segmentation_views;
/* ranges_real: W*H measured ranges, host memory or -- ranges_is_device != 0 -- device memory (_async: valid until the sync).  out may
 * be NULL (counts only); counts_out (nullable) receives {n_outlier_scan, n_outlier_map}.  Everything runs on the handle's stream: the
 * trace into the operator's own scratch, the classification, the order-preserving compaction; nothing is written beyond the counted
 * points, and the same inputs give the same bits on every run and for every find kind.  The operator's model buffers, its dataset and
 * whatever computeCrossStatistics has cached are NOT touched.  Empty model: no-op, counts 0.  NaN or negative thresholds, unknown flag
 * bits, a null Tbm / ranges_real / params: RMCLHIP_ERR_INVALID.  The _async form returns once the work is enqueued (rmclhip_rcc_sync
 * waits; the counts are then in out->counts_dev). */
rmclhip_status rmclhip_rcc_segment(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, const float* ranges_real, int ranges_is_device,
                                   const rmclhip_segmentation_params* params, const rmclhip_segmentation_views* out,
                                   uint32_t counts_out[2]);
rmclhip_status rmclhip_rcc_segment_async(rmclhip_rcc* rcc, const rmclhip_transform* Tbm, const float* ranges_real, int ranges_is_device,
                                         const rmclhip_segmentation_params* params, const rmclhip_segmentation_views* out);
/* rm::statistics_p2l(const Transform& Tpre, const PointCloudView_<MemT>& dataset, const PointCloudView_<MemT>& model,
 * const UmeyamaReductionConstraints& params) -> CrossStatistics, as a free function on CALLER-owned device views
 * (rmcl/src/rmcl/registration/CorrespondencesCUDA.cpp:28; gate and projection pinned by rmcl_ros/src/micpl/MICPSensorCPU.cpp:70-84):
 * for i < n with dataset_mask[i] > 0 && model_mask[i] > 0: Di = Tpre * dataset_points[i], d = (Ii - Di) . Ni, kept iff |d| < max_dist,
 * Mi = Di + Ni d; means of D and M, covariance 1/n sum (M - mean_M)(D - mean_D)^T, count.  Either mask may be NULL (all valid).
 * The streaming reduction of rmclhip_rcc_compute_cross_statistics (k_reduce_partials + finalize) on the context's own stream;
 * synchronous, thread-safe per context (calls on one context serialise). */
rmclhip_status rmclhip_statistics_p2l(rmclhip_ctx* ctx, const rmclhip_transform* Tpre, const float* dataset_points_xyz_dev,
                                      const uint8_t* dataset_mask_dev, const float* model_points_xyz_dev,
                                      const float* model_normals_xyz_dev, const uint8_t* model_mask_dev, uint32_t n, float max_dist,
                                      rmclhip_cross_statistics* out);

/* ---- host-side algebra (rmagine math the callers of the hot path use) -------------- */
/* rm::umeyama_transform(CrossStatistics) (micp_localization.cpp:952-953).  A covariance of rank <= 1 (s2 <= 1e-6 s1: one wall seen by a
 * 2-D lidar, two correspondences) leaves a family of optimal rotations; this returns the SHORTEST one, v1 -> u1 (the
 * rank-one rule) -- the reference's SVD returns an arbitrary member.  Zero covariance: the identity rotation. */
rmclhip_status rmclhip_umeyama_transform(const rmclhip_cross_statistics* stats, rmclhip_transform* out);
/* CrossStatistics::operator+= (micp_localization.cpp:936-937) */
rmclhip_status rmclhip_cross_statistics_merge(const rmclhip_cross_statistics* a,
                                              const rmclhip_cross_statistics* b,
                                              rmclhip_cross_statistics* out);
/* Transform * CrossStatistics (MICPSensor.hpp:182, micp_localization.cpp:931) */
rmclhip_status rmclhip_cross_statistics_transform(const rmclhip_transform* T,
                                                  const rmclhip_cross_statistics* s,
                                                  rmclhip_cross_statistics* out);
/* Transform::operator*, operator~ (micp_localization.cpp:926,963) */
rmclhip_status rmclhip_transform_mult(const rmclhip_transform* a, const rmclhip_transform* b,
                                      rmclhip_transform* out);
rmclhip_status rmclhip_transform_inv(const rmclhip_transform* a, rmclhip_transform* out);

/* ---- particle-filter sensor update (RMCL) --------------------------------------------
 * rmcl::PCDSensorUpdaterEmbree / PCDSensorUpdaterOptix
 * (rmcl_ros/src/rmcl/PCDSensorUpdaterEmbree.cpp:244-352, PCDSensorUpdaterOptix.cpp:174-350,
 *  kernels optix/BeamEvaluateProgram.cu:15-130) behind SensorUpdater<MemT>::update
 * (rmcl_ros/include/rmcl_ros/rmcl/SensorUpdater.hpp:18-42, ParticleUpdater.hpp:24-44). */
rmclhip_status rmclhip_pf_create(rmclhip_ctx* ctx, rmclhip_map* map, rmclhip_pf** out);
void rmclhip_pf_destroy(rmclhip_pf* pf);
rmclhip_status rmclhip_pf_set_params(rmclhip_pf* pf, const rmclhip_pf_params* params);
/* update(poses, attrs): all `n_beams` sampled measurements (sensor frame) are applied to every
 * particle IN ORDER, in one launch; attrs are updated in place on the device.
 * poses_dev / attrs_dev: device arrays of n_particles rmclhip_transform / rmclhip_particle_attributes. */
rmclhip_status rmclhip_pf_update(rmclhip_pf* pf, const rmclhip_transform* poses_dev,
                                 rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                 const rmclhip_range_measurement* beams, uint32_t n_beams,
                                 const rmclhip_transform* Tsb);
rmclhip_status rmclhip_pf_update_async(rmclhip_pf* pf, const rmclhip_transform* poses_dev,
                                       rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                       const rmclhip_range_measurement* beams, uint32_t n_beams,
                                       const rmclhip_transform* Tsb);
rmclhip_status rmclhip_pf_sync(rmclhip_pf* pf);
/* optional debug/parity output of the next update: per (particle, beam) error in metres
 * (device buffer of n_particles*n_beams floats, or NULL to disable) */
rmclhip_status rmclhip_pf_set_error_output(rmclhip_pf* pf, float* errors_dev);
/* MotionUpdater<MemT>::update inner loop: TFMotionUpdaterGPU / particle_move_and_forget_kernel
 * (rmcl_ros/src/rmcl/particle_motion.cu:11-46) and, with check_collision != 0, the wall-collision test the CPU
 * updater adds (TFMotionUpdaterCPU.cpp:17-50,207-221): pose <- pose * T_bnew_bold;
 * n_meas -= forget_rate * n_meas; a particle whose step crosses the mesh gets likelihood {0, 0, MAX_N_MEAS}.
 * forget_rate is the already combined rate (TFMotionUpdaterCPU.cpp:172-174), a fraction in [0, 1]: a rate outside that range, or
 * NaN, is refused with RMCLHIP_ERR_INVALID before anything is launched (the truncating store of a negative double, or of one past
 * 2^32, into the uint32 n_meas is undefined).  The same rule holds for rmclhip_pf_sharded_motion_update and, when it is given a
 * T_bnew_bold, for rmclhip_pf_sharded_step. */
rmclhip_status rmclhip_pf_motion_update(rmclhip_pf* pf, rmclhip_transform* poses_dev,
                                        rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                        const rmclhip_transform* T_bnew_bold, double forget_rate, int check_collision);
/* ---- surface-constrained motion: keep the particles of a ground robot on the mesh it drives on ----------------------------------
 * (the reference lists it as open, docs/RMCL.md:69-72: "Provide a MotionUpdater constrained to the mesh surface".)  One short ray per
 * particle; z, and with `align` roll and pitch, stop being hypotheses the sensor update has to kill.  Per particle (R, t), every
 * operation in float32 and in this order (the library is built without contraction; tests/surface_ref.py restates it in numpy):
 *   1. a = (0, 0, 1) (axis 0) or R * (0, 0, 1) (axis 1, the quaternion rotation of rmclhip_transform_mult).  Componentwise
 *      c = t - height * a (the contact point), O = c + probe_up * a, D = -a, tfar = probe_up + probe_down.
 *      A pose with a non-finite component of t or R gets no ray and counts as a miss.
 *   2. closest hit of (O, D) on (0, tfar] with the traversal's rule (min t, then min face id).  No hit: class MISS.
 *   3. n = the face's unit normal, d = (n.x * a.x + n.y * a.y) + n.z * a.z; d < 0: n = -n, d = -d (a map has no consistent winding).
 *      !(d >= min_up_cos): class STEEP.
 *   4. class SNAP: p = O + D * t_hit, t' = p + height * a (componentwise, product first).
 *   5. align: zb = R * (0, 0, 1); w = 1 + ((zb.x * n.x + zb.y * n.y) + zb.z * n.z); w < 1e-6 (upside down): q = (R * (1, 0, 0), 0), the
 *      half turn about the body's x; else q = (zb x n, w), the cross product unfused (zb.y * n.z - zb.z * n.y, ...).  normalise(q) =
 *      q / sqrt(((x * x + y * y) + z * z) + w * w), four divisions.  R' = normalise(normalise(q) (x) R): the heading changes by that
 *      shortest arc only.  (The shortest-arc construction of the rank-one Umeyama rule works in double and picks another half-turn axis;
 *      it is not shared.)
 *   6. MISS and STEEP leave the pose bit for bit; on_miss = 1 sets their likelihood to {0, 0, max_n_meas}.  state_sigma is never touched.
 * In rmclhip_pf_motion_update the constraint runs on the MOVED pose, in the same launch.  With check_collision != 0 the collision
 * segment is then lifted by the step height: it runs from O(old pose) to O(moved, not yet constrained pose) -- each with its own a --
 * so what is lower than probe_up is climbed and what is taller is a wall; length, the 1e-5 threshold and the kill are unchanged, and
 * the constraint runs whether or not the particle was killed.
 * RMCLHIP_ERR_INVALID, before anything is launched: height, probe_up or probe_down negative or not finite; min_up_cos outside [0, 1]
 * or NaN; axis, align or on_miss not 0 or 1; null buffers with n > 0. */
void rmclhip_surface_params_default(rmclhip_surface_params* out);
/* later rmclhip_pf_motion_update calls on this handle constrain in the same launch; NULL switches it off; a fresh handle has it off,
 * and every call then returns the bytes it returned before this interface existed */
rmclhip_status rmclhip_pf_set_surface(rmclhip_pf* pf, const rmclhip_surface_params* params);
/* counts of the last constrained call on the handle (motion update with the constraint set, or rmclhip_pf_constrain_to_surface);
 * zeros before the first */
rmclhip_status rmclhip_pf_get_surface_stats(rmclhip_pf* pf, rmclhip_surface_stats* out);
/* the standalone pass, e.g. after rmclhip_particles_init_uniform or a resampler's noise: steps 1-6 on n particles in place.
 * Synchronous.  stats_out nullable.  n == 0: RMCLHIP_OK, nothing touched.  max_n_meas of on_miss: the handle's rmclhip_pf_params. */
rmclhip_status rmclhip_pf_constrain_to_surface(rmclhip_pf* pf, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                               uint32_t n_particles, const rmclhip_surface_params* params,
                                               rmclhip_surface_stats* stats_out);
/* ---- MOTION NOISE: the sampled odometry model, per-particle noise that scales with the step ---------------------------------------
 * (the reference has none: its resamplers' constant noise stands in for it, ResidualResamplerCPU.cpp:92-94 "a-priori noise. how to
 * get it here?", and TFMotionUpdater.hpp:50 declares a weight_noise nobody reads.)  This is sample_motion_model_odometry with AMCL's
 * alpha1..4 spelt out per axis: every particle's step is the odometry's step composed with a Gaussian whose standard deviations grow
 * with the length and the angle of that step.  A robot that stands does not diffuse: there is deliberately no time term.
 *
 * HOST, rmclhip_motion_noise_sigma_host: everything in double from the float fields of T = T_bnew_bold,
 *   s_t = sqrt((t.x^2 + t.y^2) + t.z^2)                                        metres travelled
 *   s_r = 2 * atan2(sqrt((R.x^2 + R.y^2) + R.z^2), |R.w|)                      radians turned, in [0, pi]; q and -q give the same
 *   sigma[k]     = float(sqrt((alpha_trans_trans[k] * s_t)^2 + (alpha_trans_rot[k] * s_r)^2))     k = 0 1 2: body x y z, metres
 *   sigma[3 + k] = float(sqrt((alpha_rot_trans[k]   * s_t)^2 + (alpha_rot_rot[k]   * s_r)^2))     k = 0 1 2: roll pitch yaw, radians
 * An identity step gives six zeros.  The defaults are 0.2 throughout (AMCL's alpha1..4).  RMCLHIP_ERR_INVALID: a null argument, a
 * negative or non-finite alpha, a non-finite component of T's rotation or translation.
 *
 * DEVICE, rmclhip_pf_motion_update_noisy: rmclhip_pf_motion_update with, per particle of GLOBAL index g = first_index + i, in float32
 * unless stated (the library is built without contraction; tests/motion_noise_ref.py restates it in numpy):
 *   1. moved = pose_old * T_bnew_bold, as in rmclhip_pf_motion_update.
 *   2. A = Philox4x32-10(counter (g, step, 0, 2), key = seed), B = Philox4x32-10(counter (g, step, 1, 2), key): stream 2, so a resampler
 *      (stream 0) and an initialiser (stream 1) given the same (seed, step) draw disjoint words.  Box-Muller as in the pose
 *      initialisation (double, rounded to float): (A0, A1) -> z0, z1; (A2, A3) -> z2, z3; (B0, B1) -> z4, z5.
 *   3. N.t = (z0 * sigma[0], z1 * sigma[1], z2 * sigma[2]); N.R = EulerAngles(z3 * sigma[3], z4 * sigma[4], z5 * sigma[5]) as the pose
 *      initialisation builds it.  The noise lives in the body frame of the moved pose: forward and lateral error are different things.
 *   4. pose_new = moved * N (rmclhip_transform_mult; no normalisation afterwards, as in step 1).
 *   5. the rest runs on pose_new as rmclhip_pf_motion_update runs it on the moved pose: with check_collision the segment runs from the
 *      old position to the NOISY new one (a particle the noise pushes through a wall is killed); with the surface constraint set, the
 *      probe starts from the noisy pose and the lifted collision segment ends at its probe origin.  Forgetting is unchanged.
 * A result depends on (seed, step, g) and on the particle alone: slices called with their first_index, and any sharding, give the
 * bytes of one call on the whole cloud.  If all six sigmas are zero (+0 or -0) the call IS rmclhip_pf_motion_update: the same kernel,
 * the same bytes (a product with an exact identity would still turn a -0.0f component into +0.0f).
 * RMCLHIP_ERR_INVALID, before anything is launched and with the buffers untouched: a null handle, T_bnew_bold or sigma; a negative or
 * non-finite sigma; forget_rate outside [0, 1] or NaN; null buffers with n > 0; first_index + n above 2^32.  n == 0: RMCLHIP_OK. */
typedef struct {
  float alpha_trans_trans[3]; /* metres of body x, y, z noise per metre travelled */
  float alpha_trans_rot[3];   /* metres of body x, y, z noise per radian turned */
  float alpha_rot_trans[3];   /* radians of roll, pitch, yaw noise per metre travelled */
  float alpha_rot_rot[3];     /* radians of roll, pitch, yaw noise per radian turned */
} rmclhip_motion_noise_params;
void rmclhip_motion_noise_params_default(rmclhip_motion_noise_params* out);
rmclhip_status rmclhip_motion_noise_sigma_host(const rmclhip_motion_noise_params* params, const rmclhip_transform* T_bnew_bold,
                                               float sigma_out[6]);
rmclhip_status rmclhip_pf_motion_update_noisy(rmclhip_pf* pf, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                              uint32_t n_particles, const rmclhip_transform* T_bnew_bold, double forget_rate,
                                              int check_collision, const float sigma[6], uint64_t seed, uint32_t step,
                                              uint32_t first_index);
/* gather likelihood.mean of every particle into a dense float array (the payload of the
 * multi-GPU all-gather) */
rmclhip_status rmclhip_pf_extract_weights(rmclhip_pf* pf, const rmclhip_particle_attributes* attrs_dev,
                                          uint32_t n_particles, float* weights_dev);
/* bits 0..3: traversal (0 = while-while with the hybrid LDS + scratch stack, 1 = stack entirely in LDS, 2 = single
 * loop, A/B); bits 4..6: ray scheduling (0 = rounds of one ray per lane; 1..4 = persistent lanes that fetch the
 * next ray when 8 / 16 / 32 / 48 lanes of their wave are idle); bit 7: persistent lanes on the 128-B nodes instead
 * of their 64-B quantised twins (A/B); bit 8: the round-2 kernel on the quantised nodes (A/B); bit 9: 4096 instead of
 * 2048 rays per workgroup (A/B); bit 10: traverse the map's tree (leaves <= 4 triangles) instead of the filter's own
 * (leaves <= 2, rmclhip_bvh_build_host_pf); bit 11 (A/B, round 5): a node's children in the ray's slot order instead of sorted by
 * entry distance (measured slower: more node visits than instructions saved); bit 12 (A/B): the STORED form of rounds 3 / 4 -- every
 * beam's error kept (global scratch), a dense likelihood pass and one lane per particle walking the reference's in-order
 * Gaussian1D += chain, bit-identical to the oracle's float chain -- instead of the round-5 default, the order-independent
 * accumulation (closed-form merge weights, fixed-point accumulators: no per-beam storage, the same bits for every schedule and shard,
 * mean / sigma within 2e-6 / 5e-6 relative of the sequential chain, n_meas exact).  A fresh handle uses traversal 0,
 * refill at 48, quantised nodes of the filter's tree, sorted children, the accumulation.  The round kernels (bits 4..6 = 0,
 * bits 0..1) and the round-2 kernel (bits 7 / 8) are experiments: accepted only while librmclhip_lab.so is loaded. */
rmclhip_status rmclhip_pf_set_variant(rmclhip_pf* pf, int variant);
/* schedule of the persistent-lane kernel: a wave fetches new beams once `refill_idle_lanes` of its lanes are idle (0: the
 * threshold selected by set_variant) and leaves its node phase when at most `tail_lanes` lanes still descend while
 * another holds a leaf (default 8).  The result does not depend on either (tests/test_gpu_pf.py). */
/* Ray dealing of the sensor update.  mapping 0 (default): beam-minor -- a workgroup takes ~2048 rays of a few particles, a wave's lanes
 * hold DIFFERENT beams.  mapping 1: particle-minor -- a workgroup takes `particles_per_block` (0 = 32, at most 64) consecutive SLOTS
 * and deals their rays out so that the lanes of a wave hold the same beam of consecutive slots: nearly the same ray when the cloud has
 * converged and neighbouring slots hold neighbouring particles.  order_dev (nullable, borrowed device memory, n_order = the particle
 * count it is for): slot -> particle index, e.g. the Morton order of (x, y, yaw) (rmcl_amd.synthetic.morton_order_xy_yaw is the host
 * form tests and bench.py use); null = slot i is particle i.  The rays, every beam's error and the in-order Gaussian1D merge per
 * particle are those of mapping 0: results do not depend on the mapping or the order.
 * MEASURED NEUTRAL (round 4, profiles/r04_pf_converged_mapping.txt): on a converged cloud (sigma 0.25 m / 5 deg) mapping 1 with 16
 * slots per workgroup and the Morton order is 3 % faster than mapping 0, with larger workgroups slower -- the kernel is bound by
 * VALU issue, and coherent lanes save cache lines, not instructions.  Kept as an option; nothing selects it automatically.
 * Bit 9 of `mapping` (A/B): a workgroup's beam errors wait in LDS (rounds 3) instead of the updater's global scratch (round 4: 16 KB
 * less LDS per workgroup, 3-5 % faster, identical results; profiles/r04_pf_occupancy.txt).
 * Bit 8 of `mapping` (A/B): correspondence_type 1 (closest-point errors) WITHOUT the near-grid seed its queries start from by
 * default (room-100k: 11.7 ms seeded vs 29.7 ms; identical results). */
rmclhip_status rmclhip_pf_set_mapping(rmclhip_pf* pf, int mapping, uint32_t particles_per_block, const uint32_t* order_dev,
                                      uint32_t n_order);
rmclhip_status rmclhip_pf_set_schedule(rmclhip_pf* pf, uint32_t refill_idle_lanes, uint32_t tail_lanes);
/* Beam sampling of PCDSensorUpdater{Embree,Optix}::update (PCDSensorUpdaterEmbree.cpp:276-327) on the raw
 * sensor_msgs/PointCloud2 bytes (HOST function, no device needed): `samples` uniformly random points, each with up to 100
 * retries for one without NaN, become RangeMeasurements {orig 0, dir = p / |p|, range = |p|, cov = 0.1 I}.  The reference
 * draws from an unseeded function-static engine; here: std::mt19937(seed), index = draw % (width * height).  *n_out <
 * samples iff a sample stayed invalid (the reference returns early there). */
rmclhip_status rmclhip_pf_sample_beams_pointcloud2(const uint8_t* data, size_t nbytes, const rmclhip_pointcloud2_layout* layout,
                                                   uint32_t samples, uint64_t seed, rmclhip_range_measurement* beams_out,
                                                   uint32_t* n_out);
/* The same sampler for a scan taken in motion (HOST function; MOTION-COMPENSATED INPUT above states the pose rule): the same
 * mt19937 draws, retries and index rule, so an identity motion returns the bytes of rmclhip_pf_sample_beams_pointcloud2.  Each beam
 * gets orig = tr_i and dir = q_i * dir of its point's own pose and keeps its range.  Refusals as above, plus those of the time field
 * and the motion. */
rmclhip_status rmclhip_pf_sample_beams_pointcloud2_deskewed(const uint8_t* data, size_t nbytes,
                                                            const rmclhip_pointcloud2_layout* layout,
                                                            const rmclhip_pointcloud2_time* time, const rmclhip_scan_motion* motion,
                                                            uint32_t samples, uint64_t seed, rmclhip_range_measurement* beams_out,
                                                            uint32_t* n_out);


/* ---- resampling: rmcl::GladiatorResamplerGPU (GladiatorResamplerGPU.cpp:46-81, resampling.cu:41-219) ----
 * compute_stats: {sum, max} of likelihood.mean over n particles (simple_stats_kernel), returned to the host.
 * gladiator: champions first .. first+count-1 each fight one random enemy out of ALL n_particles; the winner
 * (enemy: copied, perturbed by the min_noise_* Gaussians, n_meas *= remember_rate) lands in
 * poses_new_dev / attrs_new_dev [0 .. count).  first/count let one GPU resample its shard of an all-gathered
 * cloud.  Random numbers: Philox4x32-10, key = seed, counter = (champion index, step, draw, 0) -- reproducible
 * and independent of the sharding (the reference's cuRAND / mt19937 streams are not reproducible).
 * The configuration of EVERY resampler below (gladiator, residual, systematic, adaptive, and the sharded resampling calls) is checked
 * before anything is launched, like the motion update's forget_rate: likelihood_forget_per_meter and likelihood_forget_per_radian are
 * fractions in [0, 1] -- outside that range pow() of a negative base is NaN --, the min_noise_* widths are finite; anything else, NaN
 * included, is refused with RMCLHIP_ERR_INVALID and the output buffers are not touched.
 * The store into the uint32 n_meas, uint32(float(n_meas) * rate), is pinned where C++ leaves the conversion undefined: NaN or a
 * product <= 0 gives 0, a product >= 2^32 gives 0xFFFFFFFF (float(n_meas) is 2^32 for every n_meas >= 2^32 - 128), anything else is
 * truncated.  That is what the CUDA reference's conversion does (resampling.cu:188); the reference's x86 CPU resamplers are undefined
 * for those values (they give 0 when built with gcc). */
rmclhip_status rmclhip_resampler_create(rmclhip_ctx* ctx, rmclhip_resampler** out);
void rmclhip_resampler_destroy(rmclhip_resampler* rs);
rmclhip_status rmclhip_resampler_compute_stats(rmclhip_resampler* rs, const rmclhip_particle_attributes* attrs_dev,
                                               uint32_t n, rmclhip_likelihood_stats* out);
/* the same {sum, max} of a DENSE weight vector on the device -- the all-gathered likelihood.mean of a sharded cloud (every
 * rank holds all N weights after the gather and computes the statistics locally, no second collective): the kernel and the order of
 * rmclhip_resampler_compute_stats, hence the same bits as that call on attributes holding the same values, on every rank */
rmclhip_status rmclhip_resampler_compute_stats_weights(rmclhip_resampler* rs, const float* weights_dev, uint32_t n,
                                                       rmclhip_likelihood_stats* out);
rmclhip_status rmclhip_resampler_gladiator(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                           const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                           rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev,
                                           uint32_t first, uint32_t count, const rmclhip_gladiator_config* config,
                                           uint64_t seed, uint32_t step);

/* rmcl::ResidualResamplerCPU::update (ResidualResamplerCPU.cpp:55-203), the PF node's second resampler plugin: until the new
 * cloud of n_new particles is full, draw a random particle and insert size_t(L / sum(L) * n_new) perturbed copies of it
 * (Gaussians of width min_noise_* / (L / max(L)); n_meas *= forget_per_meter^|dt|^2 * forget_per_radian^l2norm(dR)).  The
 * reference's loop is sequential; here the draws are a counter-based stream (draw k -> particle philox(k, step, 2)[0] % n; the
 * Gaussians of slot j from philox(j, step, 3 / 4)), so their counts, a prefix sum and the slots are three data-parallel passes
 * with the sequential loop's result.  Slots first .. first+count-1 land in poses_new_dev / attrs_new_dev [0 .. count) (a GPU
 * can fill its shard of an all-gathered cloud).  config: the gladiator's struct (trans_dist_metric is ignored).
 * n_draws_out (nullable): draws the sequential loop uses -- set when the call fills the LAST slot.  Errors: likelihoods that
 * sum to zero, to a negative value or to NaN (one NaN likelihood is enough); shares that all truncate to zero (the reference's loop
 * would not terminate).  A negative likelihood in a cloud whose sum is positive has a non-positive share and is never inserted. */
rmclhip_status rmclhip_resampler_residual(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                          const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                          rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev,
                                          uint32_t n_new, uint32_t first, uint32_t count, const rmclhip_gladiator_config* config,
                                          uint64_t seed, uint32_t step, uint64_t* n_draws_out);

/* ---- a particle count that follows the posterior: KLD-sampling bound + systematic resampling ------------------------------------
 * The reference lists it as open ("Improve strategies to reduce the number of particles more intelligently", docs/RMCL.md); its node
 * already adopts the count a resampler returns (res.n_particles, rmcl_localization.cpp:633-639).  Neither resampler above can shrink
 * a converged cloud: the gladiator keeps the count, and the residual resampler's shares size_t(L / sum * n_new) of an evenly weighted
 * cloud all truncate to zero once n_new < n.  Two parts:
 *   the size the cloud needs -- the KLD-sampling bound (Fox 2003, the rule of AMCL) from the number k of occupied bins of pose space;
 *   a resampler that produces any requested size from any weights -- systematic (low-variance) resampling.
 * Random words: the resamplers' stream (counter (index, step, draw, 0)), draws 5, 6 and 7.
 *
 * BINS.  The bin of a particle is six int32: floor(t_d / bin_xyz[d]) in float, clamped to [-8192, 8191], and floor((angle_d + pi_f) /
 * bin_rpy[d]) in float, clamped to [0, 126], for roll, pitch, yaw of the textbook ZYX extraction (float products, atan2 / asin in
 * double, rounded to float -- as the gladiator's noise step extracts them).  A bin size of 0 ignores the dimension (index 0); x, y and
 * yaw alone is AMCL's form.  A particle is counted iff its seven pose components and its likelihood.mean L are finite, L > 0 (what the
 * collision test killed never counts) and L >= min_likelihood_rel * max (float product; max = rmclhip_resampler_compute_stats's).
 * k = the number of distinct six-tuples among the counted particles: the same for every schedule and order of the cloud.
 * rmclhip_kld_params_default fills the values in brackets. */
typedef struct {
  float bin_xyz[3];          /* [0.5 0.5 0.5] metres; 0 = dimension ignored; finite, >= 0 */
  float bin_rpy[3];          /* [0.17453292 x3] radians; 0 = ignored; else >= 0.05 */
  float min_likelihood_rel;  /* [0.01] in [0, 1] */
  double epsilon;            /* [0.01] bound on the KL divergence; > 0 */
  double z;                  /* [2.3263479] upper 1 - delta quantile of N(0, 1) (delta = 0.01) */
  uint32_t n_min, n_max;     /* [500, 0xFFFFFFFF]; n_min >= 1, n_min <= n_max */
} rmclhip_kld_params;
void rmclhip_kld_params_default(rmclhip_kld_params* out);
/* k_out = occupied bins, n_counted_out (nullable) = particles that were counted.  Reads bin_xyz, bin_rpy and min_likelihood_rel of p.
 * n == 0: both 0.  The table of bins (64-bit words, a power of two >= 2 n) belongs to the handle and grows with n. */
rmclhip_status rmclhip_particles_count_bins(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                            const rmclhip_particle_attributes* attrs_dev, uint32_t n, const rmclhip_kld_params* p,
                                            uint32_t* k_out, uint32_t* n_counted_out);
/* HOST function (no device needed), in double: k < 2 gives n_min; else a = 2 / (9 (k - 1)), x = (1 - a) + sqrt(a) * z,
 * n = ceil((k - 1) / (2 epsilon) * ((x * x) * x)), clamped to [n_min, n_max] (saturating at 2^32 - 1).  RMCLHIP_ERR_INVALID: epsilon <= 0,
 * a non-finite epsilon or z, n_min == 0, n_min > n_max. */
rmclhip_status rmclhip_kld_bound_host(uint32_t k, double epsilon, double z, uint32_t n_min, uint32_t n_max, uint32_t* n_out);
/* SYSTEMATIC RESAMPLING to n_new particles.  Integer weights w_i = uint64(rint(double(L_i) / double(max) * 2^24)) (L_i negative or
 * not finite: 0), C = their inclusive 64-bit prefix sums, T = C[n - 1]: exact, whatever the launch shape.  u0 = (r[0] + 0.5) * 2^-32
 * in double, r = philox(0, step, 5, 0).  Slot j reads pos_j = min(T - 1, uint64(floor((double(j) + u0) * (double(T) / double(n_new)))));
 * its source is the first i with C[i] > pos_j.  The first slot of a run (slot 0, or source_j != source_j-1) is a bit-for-bit copy of
 * its source; every further copy is perturbed as the gladiator perturbs a winning enemy (widths min_noise_*, unscaled; the same Euler
 * step and n_meas rule, trans_dist_metric honoured), Gaussians from philox(j, step, 6, 0) and philox(j, step, 7, 0) in the gladiator's
 * word order (a[1] a[2] | a[3] b[0] | b[1] b[2]).  Hence an evenly weighted cloud resampled to its own size comes back unchanged, and
 * every particle gets within one copy of n_new * w_i / T.  Slots first .. first+count-1 land in [0, count); a call that starts at
 * first > 0 finds the source of slot first - 1 by its own search, so slices equal the whole.  Out of place.
 * RMCLHIP_ERR_INVALID: max <= 0 or not finite, n_new == 0, first + count > n_new, null buffers with count > 0.  count == 0: OK,
 * nothing touched. */
rmclhip_status rmclhip_resampler_systematic(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                            const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                            rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev,
                                            uint32_t n_new, uint32_t first, uint32_t count, const rmclhip_gladiator_config* config,
                                            uint64_t seed, uint32_t step);
/* what a Resampler::update does with res.n_particles = *n_new_out: statistics -> occupied bins -> bound, with n_max (and, where it is
 * smaller, n_min) limited by capacity_new, the particles poses_new_dev / attrs_new_dev hold -> systematic resampling to that size.
 * The result of the three calls made one after the other.  k_out: nullable. */
rmclhip_status rmclhip_resampler_adaptive(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                          const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles,
                                          rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev,
                                          uint32_t capacity_new, const rmclhip_kld_params* kld_params,
                                          const rmclhip_gladiator_config* config, uint64_t seed, uint32_t step, uint32_t* n_new_out,
                                          uint32_t* k_out);

/* ---- the particle cloud's first and last step: RmclNode::initSamplesUniform / initSamples / visualize ------------------------
 * (rmcl_ros/src/nodes/rmcl_localization.cpp:277-342, 165-275, 797-879; particle store rmcl_localization.hpp:65-77.)
 * The cloud is created ON the device: no host loop, no 68 B per particle upload.  poses_dev / attrs_dev hold particles
 * first .. first+count-1 of a cloud; element k gets the values of GLOBAL particle first+k, so a cloud is the same bits whether it
 * is filled by one call, by several calls over slices, or by the devices of a sharded filter (rmclhip_pf_sharded_init_*).
 *
 * Random words of particle i: a = Philox4x32-10(counter (i, epoch, 0, 1), key = seed), b = Philox(counter (i, epoch, 1, 1), key):
 * w0..w3 = a, w4..w5 = b[0..1].  The resamplers' counters end in 0: an initialisation and a resampler may share a seed.
 *   uniform: dimension d of x y z roll pitch yaw = float(lo_d + (hi_d - lo_d) * (w_d + 0.5) * 2^-32) in double; lo_d == hi_d gives lo_d.
 *   pose:    z = three Box-Muller pairs of w; x = float(L z) with L the factor rmclhip_chol6_host returns for `covariance`
 *            (row-major 6x6 over x y z roll pitch yaw, the layout of geometry_msgs/PoseWithCovariance); particle = Tlm * {EulerAngles
 *            (x3, x4, x5), (x0, x1, x2)}, Tlm = the pose guess in the map frame.
 * Both write the attributes the reference writes: likelihood {mean 1, sigma 0, n_meas 0}, state_sigma 0.
 * The reference's defaults are parameters of its node, not of this interface: box [-50, -50, 0, 0, 0, -pi] .. [50, 50, 0, 0, 0, pi]
 * and 50 000 particles for both initialisations (rmcl_localization.hpp:153-154, .cpp:356-359).
 * THE ONE DELIBERATE DIFFERENCE from the reference: it seeds a std::mt19937 from the clock and draws sequentially (not reproducible,
 * not parallel); here the caller passes seed and epoch, and particle i depends on (seed, epoch, i) alone -- the choice the resamplers
 * document above.  The distributions are the reference's.
 * count == 0: RMCLHIP_OK, nothing touched.  RMCLHIP_ERR_INVALID: null buffers with count > 0, bb_min[d] > bb_max[d], a non-finite bound
 * or pose, a covariance rmclhip_chol6_host refuses, first + count above 2^32.  Synchronous on return. */
rmclhip_status rmclhip_particles_init_uniform(rmclhip_ctx* ctx, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                              uint32_t first, uint32_t count, const float bb_min[6], const float bb_max[6],
                                              uint64_t seed, uint32_t epoch);
/* chol_err_out (nullable): the "Cholesky Err" the reference prints (:195), see rmclhip_chol6_host */
rmclhip_status rmclhip_particles_init_pose(rmclhip_ctx* ctx, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                           uint32_t first, uint32_t count, const rmclhip_transform* Tlm, const double covariance[36],
                                           uint64_t seed, uint32_t epoch, double* chol_err_out);
/* HOST function (no device needed): row-major lower-triangular L with L L^T = (C + C^T) / 2, computed in double and rounded to float.
 * Positive SEMIdefinite input is the normal case (RViz's /initialpose covariance has zero rows for z, roll and pitch): column by column
 * with pivot d_j = C_jj - sum_k L_jk^2 and tol = 36 * 2^-24 * max_j |C_jj|; d_j < -tol: RMCLHIP_ERR_INVALID ("not positive
 * semidefinite"); d_j <= tol: column j of L is zero; else L_jj = sqrt(d_j) and the column below it.  A non-finite entry:
 * RMCLHIP_ERR_INVALID.  err_out (nullable): sum |L L^T - C| / 36 of the float factor. */
rmclhip_status rmclhip_chol6_host(const double covariance[36], float L_out[36], double* err_out);
/* RmclNode::visualize's per-particle loop: seven dense float arrays of n, one after the other in `out` (7 * n floats; host memory, or
 * device memory with out_is_device != 0): x, y, z (pose.t), likelihood (mean), likelihood_sigma, likelihood_n_meas (float(n_meas)),
 * badness = mean * (sigma * unc + unc) with unc = float(1.0 - double(n_meas) / double(max_n_meas)) -- 28 B per particle leave the
 * device instead of 68 B and a host loop.  max_n_meas: rmclhip_pf_params::max_n_meas (the reference's MAX_N_MEAS, 10000); 0 is
 * RMCLHIP_ERR_INVALID. */
rmclhip_status rmclhip_particles_pack_visualization(rmclhip_ctx* ctx, const rmclhip_transform* poses_dev,
                                                    const rmclhip_particle_attributes* attrs_dev, uint32_t n, uint32_t max_n_meas,
                                                    float* out, int out_is_device);

/* ---- SURFACE SAMPLER: poses drawn uniformly by area on the drivable faces of the map; recovery injection -------
 * Global initialisation of a ground robot and the augmented-MCL recovery rule (Thrun, Burgard, Fox: Probabilistic Robotics, table
 * 8.3; AMCL's recovery_alpha_slow / recovery_alpha_fast) need the same primitive: a pose that stands on a face the robot can stand on,
 * every square metre of such faces equally likely -- not a 6-D box of air followed by one ray per particle
 * (rmclhip_particles_init_uniform + rmclhip_pf_constrain_to_surface), whose density follows the projected area, whose floor depends on
 * a z draw and whose draws outside the building stay where they fell.  (The reference lists neither: docs/RMCL.md.)
 *
 * THE SAMPLER, built once per (map, parameters) on the device; the handle retains the map.  Weights live on ORIGINAL FACE IDS
 * 0 .. n_faces-1 (global face ids of a scene), not on triangle records: a face the builder's spatial splits reference from k leaves
 * has k identical records and counts once, so the cloud does not depend on the tree.  Per face f, from the record with the LOWEST
 * index that carries face id f (the records of a face are identical: which one is read does not matter to the bytes):
 *   1. eligible iff |n.z| >= min_up_cos with n the record's unit normal (a map has no consistent winding: the sign is dropped; a
 *      NaN normal is not eligible) and region_min[d] <= c_d <= region_max[d] for d = x, y, z with the centroid
 *      c_d = double(v0_d) + (double(e2_d) - double(e1_d)) / 3.0 of the record's v0, e1 = v0 - v1, e2 = v2 - v0 (bounds converted to double).
 *   2. a_f = 0.5 * sqrt((double(Ng.x)^2 + double(Ng.y)^2) + double(Ng.z)^2) of the record's float Ng.
 *   3. a_max = the largest finite a_f > 0 of an eligible face (a maximum: independent of the order).
 *   4. w_f = uint64(rint(a_f / a_max * 4294967296.0)) for an eligible face with finite a_f > 0, else 0.  (A face more than 2^33 times
 *      smaller than the largest weighs 0 and is never drawn.)
 *   5. C[f] = w_0 + ... + w_f in 64 bits (the resamplers' prefix scan), T = C[n_faces - 1]: integers, exact whatever the launch shape.
 *      (w_f <= 2^32 and a map has fewer than 2^32 faces -- a face id is a 32-bit word -- so T <= (2^32 - 1) * 2^32 < 2^64: no sum wraps.)
 * No face with a positive weight: RMCLHIP_ERR_INVALID, no handle.  Refused before any launch (RMCLHIP_ERR_INVALID): min_up_cos outside
 * [0, 1] or NaN; height not finite; region_min[d] > region_max[d] or a NaN bound (infinities are allowed); yaw_min > yaw_max or either
 * not finite; align not 0 or 1; a map without faces.
 *
 * THE DRAW of one pose from two Philox blocks A, B (rmclhip_particles_init_surface and rmclhip_particles_inject_surface name their
 * counters), one function of (seed, counter) for both callers:
 *   1. r = A0 * 2^32 + A1; pos = the high 64 bits of the 128-bit product r * T: uniform on [0, T).  The face is the first f with
 *      C[f] > pos; its record is the one of step "per face" above.
 *   2. u = (A2 + 0.5) * 2^-32, v = (A3 + 0.5) * 2^-32 in double; u + v > 1.0: u = 1.0 - u, v = 1.0 - v.
 *      p_d = float((double(v0_d) - u * double(e1_d)) + v * double(e2_d)): the point v0 + u (v1 - v0) + v (v2 - v0).
 *   3. yaw = float(double(yaw_min) + (double(yaw_max) - double(yaw_min)) * (B0 + 0.5) * 2^-32), the rule of the uniform initialisation;
 *      R = Quaternion(EulerAngles(0, 0, yaw)) by that initialisation's conversion.
 *   4. n = the record's unit normal, negated when n.z < 0.  a = (0, 0, 1) (align 0) or n (align 1).
 *   5. align 1: R = step 5 of the surface constraint above applied to (R, n): the shortest arc that takes the body's z onto n, its
 *      float arithmetic, its w < 1e-6 half turn about the body's x and its two normalisations.
 *   6. t_d = p_d + height * a_d in float, the product first.  stamp = 0.
 * Every operation is IEEE in this order (the library is built without contraction); tests/surface_sample_ref.py restates it. */
typedef struct {
  float min_up_cos;                   /* [0.7] */
  float height;                       /* [0]  the pose stands this far above the face, along a */
  int align;                          /* [0]  0: roll = pitch = 0; 1: body z on the (flipped) face normal */
  float region_min[3], region_max[3]; /* [-inf, +inf] */
  float yaw_min, yaw_max;             /* [-pi_f, pi_f], pi_f = float(pi) */
} rmclhip_surface_sample_params;
typedef struct {
  uint32_t n_faces;        /* of the map */
  uint32_t n_eligible;     /* faces that pass rule 1 */
  uint32_t n_weighted;     /* faces with w_f > 0 */
  uint32_t reserved;
  double area_eligible;    /* the a_f of the eligible faces with a finite area, added in double in increasing face id (on the host) */
  uint64_t weight_total;   /* T */
} rmclhip_surface_sample_info;
typedef struct rmclhip_surface_sampler rmclhip_surface_sampler;
void rmclhip_surface_sample_params_default(rmclhip_surface_sample_params* out);
/* params NULL: the defaults.  Synchronous. */
rmclhip_status rmclhip_surface_sampler_create(rmclhip_map* map, const rmclhip_surface_sample_params* params, rmclhip_surface_sampler** out);
void rmclhip_surface_sampler_destroy(rmclhip_surface_sampler* sampler);
rmclhip_status rmclhip_surface_sampler_get_info(const rmclhip_surface_sampler* sampler, rmclhip_surface_sample_info* out);
/* Initialisation on the surface.  Global particle i = first + k draws from A = Philox(counter (i, epoch, 2, 1), key = seed),
 * B = Philox(counter (i, epoch, 3, 1), key) -- stream 1 of the initialisations, behind their draws 0 and 1.  Attributes and contract
 * are rmclhip_particles_init_uniform's: likelihood {1, 0, 0}, state_sigma 0; element k holds global particle first + k, so slices and
 * shards equal the whole; count == 0 is RMCLHIP_OK with nothing touched; RMCLHIP_ERR_INVALID for a null sampler, null buffers with
 * count > 0 or first + count above 2^32 (RMCLHIP_ERR_UNSUPPORTED above 2^32 / 9 particles in one call).  Synchronous on return. */
rmclhip_status rmclhip_particles_init_surface(rmclhip_surface_sampler* sampler, rmclhip_transform* poses_dev,
                                              rmclhip_particle_attributes* attrs_dev, uint32_t first, uint32_t count, uint64_t seed,
                                              uint32_t epoch);
/* RECOVERY (augmented MCL as AMCL runs it): a slow and a fast running average of the cloud's mean likelihood; when the fast one
 * drops below the slow one, the fraction p = 1 - w_fast / w_slow of the cloud is replaced by fresh draws from the sampler.
 * rmclhip_recovery_update_host -- a HOST function, no device needed, in double, in this order:
 *   avg = likelihood_sum / double(n);
 *   w_slow == 0: w_slow = avg, else w_slow = w_slow + alpha_slow * (avg - w_slow);  the same for w_fast with alpha_fast;
 *   p = 0 while !(w_slow > 0), else p = 1.0 - w_fast / w_slow clamped to [0, p_max] (below 0 or NaN: 0).
 * RMCLHIP_ERR_INVALID, state untouched: null state or params; an alpha outside (0, 1] or NaN; alpha_slow > alpha_fast; p_max outside
 * [0, 1] or NaN; n == 0; a likelihood_sum that is negative or not finite.  p_inject_out is nullable.
 * rmclhip_recovery_reset_host zeroes both averages: AMCL does so after it has injected, so one drop does not inject forever.
 * The defaults {0.001, 0.1, 1.0} are AMCL's recovery_alpha_slow / recovery_alpha_fast; they are not tuned here. */
typedef struct { double w_slow, w_fast; } rmclhip_recovery_state;                    /* zeros = fresh */
typedef struct { double alpha_slow, alpha_fast; double p_max; } rmclhip_recovery_params;
void rmclhip_recovery_params_default(rmclhip_recovery_params* out);
rmclhip_status rmclhip_recovery_update_host(rmclhip_recovery_state* state, const rmclhip_recovery_params* params, double likelihood_sum,
                                            uint32_t n, double* p_inject_out);
rmclhip_status rmclhip_recovery_reset_host(rmclhip_recovery_state* state);
/* Injection, in place on particles first .. first+count-1 of a cloud any resampler (or a shard of one) produced.  Slot j = first + k
 * is replaced iff uint64(Philox(counter (j, step, 9, 0), key = seed)[0]) < uint64(floor(p_inject * 4294967296.0)): p_inject 1 replaces
 * every slot; a threshold of 0 (p_inject below 2^-32) launches nothing and touches nothing.  A replaced slot gets THE DRAW with
 * A = Philox(counter (j, step, 10, 0), key), B = Philox(counter (j, step, 11, 0), key) -- stream 0 of the resamplers, behind their
 * draws 0..8, so an injection shares seed and step with the resampler it follows -- and the initialisation's attributes (an unmeasured
 * particle: its first sensor update replaces its likelihood).  Every other slot keeps its bytes.  n_injected_out (nullable): replaced
 * slots of this call.  RMCLHIP_ERR_INVALID, nothing touched: p_inject outside [0, 1] or NaN, and rmclhip_particles_init_surface's
 * refusals.  count == 0: RMCLHIP_OK.  Synchronous on return. */
rmclhip_status rmclhip_particles_inject_surface(rmclhip_surface_sampler* sampler, rmclhip_transform* poses_dev,
                                                rmclhip_particle_attributes* attrs_dev, uint32_t first, uint32_t count, double p_inject,
                                                uint64_t seed, uint32_t step, uint32_t* n_injected_out);

/* ---- multi-GPU: ONE process drives several devices -------------------------------------------------------------
 * (the reference's localisation node is one process: rmcl_localization.cpp:482-552; particle store rmcl_localization.hpp:65-77.
 * The reference has no distributed code -- SURVEY.md 8(e) defines this part.)  Particles are block-partitioned over the
 * devices, mesh + BVH are replicated (built once), beams are identical everywhere; exchanges are RCCL collectives over xGMI
 * (librccl is loaded with dlopen by rmclhip_comm_create: single-GPU users never touch it). */
/* devices: HIP device indices (NULL = 0 .. ndev-1).  ncclCommInitAll. */
rmclhip_status rmclhip_comm_create(const int* devices, uint32_t ndev, rmclhip_comm** out);
/* TEST INFRASTRUCTURE: an in-process stand-in for the RCCL communicator -- same handle type, accepted by every rmclhip_pf_sharded_*
 * entry point; every "rank" is a stream of this process and `devices` may repeat a device; an all-gather is device-to-device
 * copies, an all-reduce one small kernel, ordered with events.  It lets the ndev > 1 code paths (grouped all-gather of weights and of
 * the cloud, the moment all-reduces, the per-rank tournament / residual fill) run, and be checked against the unsharded results,
 * on a box with ONE GPU; it is not a transport (no xGMI, no peer access set-up). */
rmclhip_status rmclhip_comm_create_loopback(const int* devices, uint32_t ndev, rmclhip_comm** out);
void rmclhip_comm_destroy(rmclhip_comm* comm);
uint32_t rmclhip_comm_size(const rmclhip_comm* comm);
/* contiguous block partition of [0, n): rank owns [lo, hi); the first n % world ranks own one extra element */
void rmclhip_shard_bounds(uint32_t n, uint32_t rank, uint32_t world, uint32_t* lo, uint32_t* hi);
/* one context + map replica + sensor updater + resampler per device of the communicator */
rmclhip_status rmclhip_pf_sharded_create(rmclhip_comm* comm, const float* vertices_xyz, uint32_t n_vertices,
                                         const uint32_t* faces_ijk, uint32_t n_faces, rmclhip_pf_sharded** out);
void rmclhip_pf_sharded_destroy(rmclhip_pf_sharded* pf);
rmclhip_status rmclhip_pf_sharded_set_params(rmclhip_pf_sharded* pf, const rmclhip_pf_params* params);
/* scatter the (host) cloud: rank r receives particles [lo_r, hi_r) */
rmclhip_status rmclhip_pf_sharded_set_particles(rmclhip_pf_sharded* pf, const rmclhip_transform* poses,
                                                const rmclhip_particle_attributes* attrs, uint32_t n_total);
/* (re)create a sharded cloud of n particles in place on its devices: every device fills its own block (rmclhip_shard_bounds) with
 * rmclhip_particles_init_uniform / _pose's values of its global indices -- the single-device cloud bit for bit, no upload, no
 * collective; all devices' launches are enqueued before the host waits for any.  Buffers are sized as by
 * rmclhip_pf_sharded_set_particles; afterwards download, step and the rest work as after that call. */
rmclhip_status rmclhip_pf_sharded_init_uniform(rmclhip_pf_sharded* pf, uint32_t n, const float bb_min[6], const float bb_max[6],
                                               uint64_t seed, uint32_t epoch);
rmclhip_status rmclhip_pf_sharded_init_pose(rmclhip_pf_sharded* pf, uint32_t n, const rmclhip_transform* Tlm, const double covariance[36],
                                            uint64_t seed, uint32_t epoch, double* chol_err_out);
rmclhip_status rmclhip_pf_sharded_download(rmclhip_pf_sharded* pf, rmclhip_transform* poses, rmclhip_particle_attributes* attrs);
/* PCDSensorUpdater*::update on every device's block (concurrently), then rmclhip_pf_allgather_weights */
rmclhip_status rmclhip_pf_update_sharded(rmclhip_pf_sharded* pf, const rmclhip_range_measurement* beams, uint32_t n_beams,
                                         const rmclhip_transform* Tsb);
/* MotionUpdater<MemT>::update on every device's block (rmcl_localization.cpp:432-480; particle_move_and_forget_kernel,
 * rmcl_ros/src/rmcl/particle_motion.cu:11-46, with check_collision != 0 also the wall-collision ray of TFMotionUpdaterCPU.cpp:17-50,
 * 207-221): the arguments of rmclhip_pf_motion_update, applied to the whole sharded cloud in place -- one launch per device, all
 * enqueued before the host waits for any.  Identical to rmclhip_pf_motion_update on the unsharded cloud (a particle's result depends on
 * that particle alone). */
rmclhip_status rmclhip_pf_sharded_motion_update(rmclhip_pf_sharded* pf, const rmclhip_transform* T_bnew_bold, double forget_rate,
                                                int check_collision);
/* the motion noise on a sharded cloud (MOTION NOISE above): rmclhip_pf_motion_update_noisy on every device's block, each with the
 * global index of its first particle as first_index -- the single-device call on the whole cloud, bit for bit, whatever the number of
 * devices.  The same refusals, before any device is touched. */
rmclhip_status rmclhip_pf_sharded_motion_update_noisy(rmclhip_pf_sharded* pf, const rmclhip_transform* T_bnew_bold, double forget_rate,
                                                      int check_collision, const float sigma[6], uint64_t seed, uint32_t step);
/* later rmclhip_pf_sharded_step calls that are given a T_bnew_bold derive sigma from these parameters and that step
 * (rmclhip_motion_noise_sigma_host) and draw with their own `seed` and `step` arguments: stream 2, disjoint from the resampler's draws
 * of the same cycle.  NULL switches it off; a fresh handle has it off and returns the bytes it returned before this interface existed.
 * RMCLHIP_ERR_INVALID: parameters rmclhip_motion_noise_sigma_host refuses (the previous setting stays); a step then refuses a
 * T_bnew_bold that function refuses, before anything is launched. */
rmclhip_status rmclhip_pf_sharded_set_motion_noise(rmclhip_pf_sharded* pf, const rmclhip_motion_noise_params* params);
/* the surface constraint on a sharded cloud: rmclhip_pf_sharded_motion_update and rmclhip_pf_sharded_step honour the setting (NULL
 * switches it off); the standalone pass runs on every device's own block, no collective; the devices' counts are summed on the host.
 * Equal, bit for bit, to the single-device calls.  rmclhip_pf_sharded_get_surface_stats: the sum over the devices' last constrained
 * launch (after a motion update, a step or the standalone pass has returned). */
rmclhip_status rmclhip_pf_sharded_set_surface(rmclhip_pf_sharded* pf, const rmclhip_surface_params* params);
rmclhip_status rmclhip_pf_sharded_constrain_to_surface(rmclhip_pf_sharded* pf, const rmclhip_surface_params* params,
                                                       rmclhip_surface_stats* stats_out);
rmclhip_status rmclhip_pf_sharded_get_surface_stats(rmclhip_pf_sharded* pf, rmclhip_surface_stats* out);
/* the surface sampler on a sharded cloud: one sampler per map replica (params NULL drops them; a refusal leaves the previous ones).
 * rmclhip_pf_sharded_init_surface (re)creates a cloud of n particles as rmclhip_pf_sharded_init_uniform does, every device filling its
 * own block with rmclhip_particles_init_surface's values of its global indices; rmclhip_pf_sharded_inject_surface replaces slots of
 * every device's block in place.  No collective; all devices' launches are enqueued before the host waits for any; the injected counts
 * are summed on the host (n_injected_out nullable).  Equal, bit for bit, to the single-device calls on the whole cloud.
 * RMCLHIP_ERR_INVALID without samplers. */
rmclhip_status rmclhip_pf_sharded_set_surface_sampler(rmclhip_pf_sharded* pf, const rmclhip_surface_sample_params* params);
rmclhip_status rmclhip_pf_sharded_init_surface(rmclhip_pf_sharded* pf, uint32_t n, uint64_t seed, uint32_t epoch);
rmclhip_status rmclhip_pf_sharded_inject_surface(rmclhip_pf_sharded* pf, double p_inject, uint64_t seed, uint32_t step,
                                                 uint32_t* n_injected_out);
/* One cycle of the filter node on the sharded cloud (rmcl_localization.cpp:84, 432-552): motion update (T_bnew_bold NULL: skipped) ->
 * sensor update -> weight all-gather -> {sum, max} of the gathered weights on every device (stats_out, nullable; no collective) -> resampling (resample: 0 none, 1 gladiator
 * tournament, 2 residual; config / seed / step as rmclhip_pf_sharded_resample).  A device's motion and sensor-update launches share a
 * stream: the host never waits between them.  Equal, bit for bit, to the single-device sequence rmclhip_pf_motion_update,
 * rmclhip_pf_update, rmclhip_resampler_compute_stats, rmclhip_resampler_gladiator / _residual. */
rmclhip_status rmclhip_pf_sharded_step(rmclhip_pf_sharded* pf, const rmclhip_transform* T_bnew_bold, double forget_rate, int check_collision,
                                       const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                       int resample, const rmclhip_gladiator_config* config, uint64_t seed, uint32_t step,
                                       rmclhip_likelihood_stats* stats_out);
/* ONE ncclAllGather of likelihood.mean (4 B x N on equal padded shards): afterwards every device holds the dense weight
 * vector of the whole cloud; rmclhip_pf_sharded_get_weights copies rank's copy to the host */
rmclhip_status rmclhip_pf_allgather_weights(rmclhip_pf_sharded* pf);
rmclhip_status rmclhip_pf_sharded_get_weights(rmclhip_pf_sharded* pf, uint32_t rank, float* weights_host);
/* global {sum, max} (simple_stats_kernel, resampling.cu:41-92).  Since round 6 NOT a collective, the name notwithstanding: after the
 * weight all-gather every device holds all N likelihoods and reduces its own copy with the single-device kernel in that kernel's fixed
 * order -- the single-device value bit for bit, independent of the order in which a collective library would have added per-device
 * partials (the value feeds size_t(L / sum * N) in the residual resampler).  Gathers first if the attributes changed since the last gather. */
rmclhip_status rmclhip_pf_allreduce_stats(rmclhip_pf_sharded* pf, rmclhip_likelihood_stats* out);
/* ranks the communicator's collectives span, as the collective library itself reports them (ncclCommCount; the loopback stand-in: its
 * rank list) and whether it is RCCL (1) or the stand-in (0) */
rmclhip_status rmclhip_comm_collective_ranks(rmclhip_comm* comm, uint32_t* n_ranks, int* is_rccl);
/* RmclNode::estimateStats (rmcl_localization.cpp:642-731) over the first n_induction particles: three passes of per-device
 * moments (<= 24 doubles each: likelihood sums + bounding box, weighted quaternion outer products + translations for the
 * Markley mean, 6x6 covariance around it), each followed by one ncclAllReduce.  A cloud whose first n_induction likelihoods sum
 * to zero (every particle killed by the collision test) or to NaN has no weighted mean: RMCLHIP_ERR_INVALID ("sum to zero"), *out
 * zeroed, as rmclhip_resampler_residual refuses the same cloud. */
rmclhip_status rmclhip_pf_allreduce_pose_estimate(rmclhip_pf_sharded* pf, uint32_t n_induction, rmclhip_pose_estimate* out);
/* distributed GladiatorResamplerGPU::update: all-gather of the 68-B particle records, then every device resamples its own
 * champions against the gathered cloud (Philox counter = GLOBAL champion index => identical to one GPU).  A particle count
 * that is not a multiple of the device count gathers padded shards and squeezes them dense on every device first. */
rmclhip_status rmclhip_pf_sharded_resample(rmclhip_pf_sharded* pf, const rmclhip_gladiator_config* config, uint64_t seed, uint32_t step);
/* the same exchange with the residual resampler (rmclhip_resampler_residual): every device fills its slots of the new cloud from the
 * gathered one -- identical to one GPU (draws and Gaussians are functions of global indices) */
rmclhip_status rmclhip_pf_sharded_resample_residual(rmclhip_pf_sharded* pf, const rmclhip_gladiator_config* config, uint64_t seed, uint32_t step);

/* ---- pose hypotheses: the clusters of the cloud's occupied bins ------------------------------------------------------------------
 * While the posterior still has two or more modes (a symmetric corridor, a repeated room: the phase uniform initialisation and the
 * KLD bound exist for), the one Markley mean of estimateStats lies between them.  AMCL, whose bound is adopted above, answers with
 * cluster statistics: group the occupied bins, weigh each group, report the heaviest group's mean and covariance.  Every quantity
 * marked EXACT is the same for every launch shape, every order of the cloud and every shard count.
 *
 * BINS.  rmclhip_particles_count_bins's: the same six fields, clamps, ignored dimensions, counted-particle rule and likelihood floor
 * min_likelihood_rel * max (max = rmclhip_resampler_compute_stats's).  A particle that is not counted belongs to no bin and no cluster;
 * a bin that only uncounted particles fall into does not exist and joins nothing.  The 63-bit key of a bin: (x + 8192) | (y + 8192) << 14
 * | (z + 8192) << 28 | roll << 42 | pitch << 49 | yaw << 56.
 * ADJACENCY.  Two occupied bins are neighbours iff they are adjacent in every one of the six fields.  x, y, z and pitch: |i - j| <= 1.
 * roll and yaw, which wrap: |i - j| <= 1, or min(i, j) == 0 && max(i, j) >= last - 1, last = the index the bin rule gives the angle pi_f
 * (floor((3.14159265f + pi_f) / width) in float, clamped).  The last - 1 is deliberate: with the default 10 degree width `last` is a sliver
 * bin that holds +pi alone, and the particles just below +pi sit in last - 1.  An ignored dimension has a constant index and never
 * separates bins; a rule with d active fields has 3^d - 1 neighbours per bin (a few more at the wrap).
 * CLUSTERS.  The connected components of that graph.  key_min: the smallest key among a cluster's bins, its id (EXACT).  n_bins and
 * estimate.n_particles: its bins and its counted particles (EXACT).  weight: the sum over its counted particles of the systematic
 * resampler's integer weight uint64(rint(double(L_i) / double(max) * 2^24)) (EXACT).  weight_share: double(weight) / double(total weight
 * of all counted particles).
 * ORDER.  By weight descending, then key_min ascending (keys are distinct: a total order).  Hypothesis r is the cluster of rank r, for
 * r < min(max_hypotheses, n_clusters).
 * ESTIMATE.  A rmclhip_pose_estimate filled as rmclhip_pf_allreduce_pose_estimate fills it, over the cluster's counted particles alone,
 * in ascending particle index, without an n_induction cut: likelihood statistics and translation box, the Markley mean with weights
 * L_i / L_sum (L_sum the cluster's own sum, in double), the covariance around that mean.
 * LABELS.  Optional device uint32[n]: entry i = the rank of particle i's cluster if that rank is below max_hypotheses, else
 * 0xFFFFFFFF; uncounted particles get 0xFFFFFFFF (EXACT). */
typedef struct {
  rmclhip_pose_estimate estimate;
  uint64_t key_min, weight;
  double weight_share;
  uint32_t n_bins, reserved;
} rmclhip_pose_hypothesis;
/* RmclNode::estimateStats (rmcl_localization.cpp:642-731) over the first min(n, n_induction) particles of a cloud on ONE device:
 * rmclhip_pf_allreduce_pose_estimate on a one-rank sharded filter, bit for bit (the same kernels and the same host code), its
 * refusals included: RMCLHIP_ERR_INVALID "no particles" (n or n_induction 0), "sum to zero".  *out is zeroed first.  Synchronous. */
rmclhip_status rmclhip_particles_pose_estimate(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                               const rmclhip_particle_attributes* attrs_dev, uint32_t n, uint32_t n_induction,
                                               rmclhip_pose_estimate* out);
/* Reads bin_xyz, bin_rpy and min_likelihood_rel of bins (checked as count_bins checks them).  max_hypotheses in [1, 64], else
 * RMCLHIP_ERR_INVALID; out holds max_hypotheses records, the first *n_out = min(max_hypotheses, *n_clusters_out) are written.  n == 0 or
 * no counted particle (a maximum <= 0 or not finite included): RMCLHIP_OK, both counts 0, nothing written to out, labels all
 * 0xFFFFFFFF.  At most 2^30 particles.  The scratch belongs to the handle and grows as the bin table does; a later
 * rmclhip_particles_count_bins / rmclhip_resampler_adaptive on the handle returns what it returned before.  Synchronous. */
rmclhip_status rmclhip_particles_pose_hypotheses(rmclhip_resampler* rs, const rmclhip_transform* poses_dev,
                                                 const rmclhip_particle_attributes* attrs_dev, uint32_t n, const rmclhip_kld_params* bins,
                                                 uint32_t max_hypotheses, rmclhip_pose_hypothesis* out, uint32_t* n_out,
                                                 uint32_t* n_clusters_out, uint32_t* labels_dev /* nullable */);
/* the sharded cloud's hypotheses: the particle records are gathered as rmclhip_pf_sharded_resample gathers them, then the
 * single-device path runs on rank 0's gathered copy -- the single-device bytes.  The cloud is not changed. */
rmclhip_status rmclhip_pf_sharded_pose_hypotheses(rmclhip_pf_sharded* pf, const rmclhip_kld_params* bins, uint32_t max_hypotheses,
                                                  rmclhip_pose_hypothesis* out, uint32_t* n_out, uint32_t* n_clusters_out);

/* ---- POSE COVARIANCE: the point-to-plane information matrix of a correction's correspondences -----------------------------------
 * MICPLocalizationNode::publishPose (micp_localization.cpp:1062-1076) fills the covariance of the PoseWithCovarianceStamped it
 * publishes with (1 - convergence_progress) + pose_noise on the diagonal -- "just some bad guess of the covariance".  The quantity
 * that tells a corridor from a room is the 6 x 6 normal matrix of the point-to-plane problem over the correspondences the
 * correction used.  It is fourth order in the data: CrossStatistics and the published moments do not contain it.
 *
 * CORRESPONDENCES.  Exactly those of rmclhip_statistics_p2l: both masks non-zero (a NULL mask: all valid), Di = Tpre * dataset_points[i]
 * and r_i = (Ii - Di) . Ni in f32 by the arithmetic of that reduction, kept iff |r_i| < max_dist (strict).  n_meas therefore EQUALS
 * the n_meas of rmclhip_statistics_p2l on the same inputs, always.  A masked-out or rejected element does not touch the sums (a miss's
 * NaN point and normal included).
 * SUMS.  In double, from the f32 values Di, Ni, r_i: u_i = [ Ni ; Di x Ni ; r_i ] (7 values).  A small motion xi = (dt, dtheta) of the
 * dataset points in their own frame, D' = D + dt + dtheta x D, changes the residual to r_i - J_i xi with J_i = u_i[0:6], so
 *   A = sum J_i^T J_i   (6 x 6, symmetric, row-major; order x y z rot-x rot-y rot-z: geometry_msgs' covariance order to first order)
 *   g = sum J_i^T r_i   (6)          rss = sum r_i^2          n_meas
 * -- the 28 distinct entries of sum u_i u_i^T and the count.  trace(A[0:3, 0:3]) / n_meas = 1 (unit normals).  The Gauss-Newton step
 * is A xi = g.  Summation order is fixed: the same inputs give the same bytes on every call. */
typedef struct { double A[36]; double g[6]; double rss; uint32_t n_meas; uint32_t pad; } rmclhip_pose_information;
/* the twin of rmclhip_statistics_p2l on caller-owned device views: same arguments, same stream and scratch owner (the context), synchronous,
 * calls on one context serialise.  n == 0: all zeros. */
rmclhip_status rmclhip_pose_information_p2l(rmclhip_ctx* ctx, const rmclhip_transform* Tpre, const float* dataset_points_xyz_dev,
                                            const uint8_t* dataset_mask_dev, const float* model_points_xyz_dev,
                                            const float* model_normals_xyz_dev, const uint8_t* model_mask_dev, uint32_t n, float max_dist,
                                            rmclhip_pose_information* out);
/* the twin of rmclhip_rcc_compute_cross_statistics after a find: the operator's dataset against its model buffers, sensor frame,
 * max_dist' = max_dist (1 - convergence_progress) + adaptive_max_dist_min convergence_progress.  RMCLHIP_ERR_INVALID when no find has
 * run, when the last find was a batch, or when rmclhip_rcc_set_outputs deselected hits, points or normals.  Only reads buffers: the
 * published moment set, rmclhip_ccs_info and what rmclhip_rcc_compute_cross_statistics returns are untouched.  Synchronous. */
rmclhip_status rmclhip_rcc_pose_information(rmclhip_rcc* rcc, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                            rmclhip_pose_information* out);
/* after rmclhip_rcc_find_batch / rmclhip_rcc_correct_batch of nposes poses: out[nposes], pose p's model buffers against the shared
 * dataset with the identity pre-transform.  RMCLHIP_ERR_INVALID when nposes is not what the last find held (and as above).  After a
 * single find that is nposes == 1: the batch form then equals rmclhip_rcc_pose_information with the identity pre-transform. */
rmclhip_status rmclhip_rcc_pose_information_batch(rmclhip_rcc* rcc, uint32_t nposes, double convergence_progress,
                                                  rmclhip_pose_information* out);
/* ---- host algebra on rmclhip_pose_information (double; out may alias an input) ----
 * Frame change, the role rmclhip_cross_statistics_transform has: with T = (R, t), J' = [R n ; R (D x n) + t x R n], so with
 * X = [[R, 0], [[t]x R, R]]: A' = X A X^T, g' = X g; rss and n_meas are unchanged.  R is the rotation of T's quaternion normalised in
 * double (a float32 quaternion is a unit one to 1e-7 only); a zero or non-finite quaternion: RMCLHIP_ERR_INVALID. */
rmclhip_status rmclhip_pose_information_transform(const rmclhip_transform* T, const rmclhip_pose_information* in,
                                                  rmclhip_pose_information* out);
/* out = a + weight_b * b for A, g and rss (micp_localization.cpp:936-944, merge_weight_multiplier); n_meas adds unscaled.
 * weight_b must be finite and >= 0. */
rmclhip_status rmclhip_pose_information_merge(const rmclhip_pose_information* a, const rmclhip_pose_information* b, double weight_b,
                                              rmclhip_pose_information* out);
/* xi = A^+ g, the Gauss-Newton step (a cross-check against rmclhip_umeyama_transform).  A^+: the pseudo-inverse from the symmetric
 * eigen-decomposition (cyclic Jacobi), eigenvalues <= rcond * lambda_max dropped. */
rmclhip_status rmclhip_pose_information_solve_host(const rmclhip_pose_information* in, double rcond, double xi_out[6]);
typedef struct {
  double sigma;                /* range noise (m); <= 0: estimated from the residuals, s2 = rss / (n_meas - 6), which needs n_meas > 6 */
  double rcond;                /* an eigenvalue of A <= rcond * lambda_max is a direction the scan does not constrain */
  double degenerate_variance;  /* the variance reported along such a direction */
  double min_eig_trans, min_eig_rot;   /* thresholds of the degeneracy report (eigenvalues of the diagonal blocks of A / n_meas) */
} rmclhip_pose_covariance_params;
typedef struct {
  double covariance[36];       /* V diag(c_k) V^T, (lambda_k, V) the eigenpairs of A, c_k = s2 / lambda_k where lambda_k > rcond * lambda_max,
                                * else degenerate_variance; row-major, the order of A */
  double eig_trans[3], eigvec_trans[9];   /* eigenpairs of A[0:3, 0:3] / n_meas, ascending; eigenvector k = eigvec_trans[3 k .. 3 k + 2] */
  double eig_rot[3], eigvec_rot[9];       /* the same of A[3:6, 3:6] / n_meas (m^2: depends on where the frame's origin lies) */
  uint32_t n_degenerate_trans, n_degenerate_rot;   /* block eigenvalues below min_eig_trans / min_eig_rot */
  double s2;                   /* the residual variance used */
} rmclhip_pose_covariance;
/* sigma 0 (estimated), rcond 1e-9, degenerate_variance 1e6, min_eig_trans 1e-3, min_eig_rot 1e-3 */
void rmclhip_pose_covariance_params_default(rmclhip_pose_covariance_params* out);
/* RMCLHIP_ERR_INVALID: sigma <= 0 with n_meas <= 6, a negative or non-finite rcond / degenerate_variance, non-finite entries of A.
 * n_meas == 0 with sigma > 0: every direction is degenerate. */
rmclhip_status rmclhip_pose_covariance_host(const rmclhip_pose_information* in, const rmclhip_pose_covariance_params* p,
                                            rmclhip_pose_covariance* out);

/* ---- ROBUST MICP: M-estimator weights in the point-to-plane reduction ----------------------------------------------
 * rmclhip_statistics_p2l trusts a correspondence fully (|r| < max_dist) or not at all.  Here every gated-in correspondence enters the
 * 16 sums with a weight w(r) in [0, 1] of its own residual, and a correction iterates reduction and solve with the weights re-evaluated
 * at every pre-transform (iteratively reweighted least squares).
 *
 * RESIDUAL.  r_i = (Ii - Di) . Ni in f32, Di = Tpre * dataset_points[i]: the value rmclhip_statistics_p2l gates on, by the same f32
 * expressions.  The hard gate |r_i| < max_dist comes first (a NaN r fails it); masked or gated-out elements have weight 0 and touch no sum.
 * WEIGHTS, all in f32 with IEEE division and no fused operation, u = r / c for a scale c > 0:
 *   NONE 1 | HUBER |r| <= c ? 1 : c / |r| | CAUCHY 1 / (1 + u u) | TUKEY |r| < c ? (1 - u u)^2 : 0 | GEMAN_MCCLURE 1 / ((1 + u u)(1 + u u))
 * r = 0 gives 1 for every kernel.  numpy float32 reproduces every weight bit for bit.
 * SCALE.  FIXED: c = scale.  MAD: c = max((float)(tuning * 1.4826 * (double)median), scale_min), median = the exact lower median of
 * |r| over the m gated-in correspondences (element (m - 1) / 2 of the sorted values; radix selection on the device, integers only: the
 * same inputs give the same value whatever the schedule); m == 0: c = scale_min.
 * SUMS.  The 16 sums of rmclhip_statistics_p2l with every term multiplied by (double)w, same grid, same order of additions: with weight
 * 1 throughout, `stats` equals rmclhip_statistics_p2l's bytes.  The means and the covariance divide by weight_sum; n_meas is the number
 * of gated-in correspondences (the covariance is zeroed when that is 1); weight_sum == 0 leaves means and covariance zero. */
enum {
  RMCLHIP_ROBUST_NONE = 0, RMCLHIP_ROBUST_HUBER = 1, RMCLHIP_ROBUST_CAUCHY = 2, RMCLHIP_ROBUST_TUKEY = 3, RMCLHIP_ROBUST_GEMAN_MCCLURE = 4
};
enum { RMCLHIP_ROBUST_SCALE_FIXED = 0, RMCLHIP_ROBUST_SCALE_MAD = 1 };
typedef struct rmclhip_robust_params {
  int32_t kernel;        /* RMCLHIP_ROBUST_* */
  int32_t scale_mode;    /* RMCLHIP_ROBUST_SCALE_FIXED | RMCLHIP_ROBUST_SCALE_MAD */
  float scale;           /* FIXED: c itself */
  float tuning;          /* MAD: c = tuning * 1.4826 * median|r| */
  float scale_min;       /* MAD: floor of c (a perfect synthetic scan has median 0) */
  uint32_t reserved;
} rmclhip_robust_params;
typedef struct rmclhip_robust_statistics {
  rmclhip_cross_statistics stats;   /* weighted means and covariance; n_meas = gated-in count */
  double weight_sum, wrss, rss;     /* sum w, sum w r^2, sum r^2 (r widened to double before squaring) */
  float scale;                      /* the c that was used */
  float median_abs_residual;        /* MAD mode, else 0 */
} rmclhip_robust_statistics;
/* MAD, the kernel's customary tuning (HUBER 1.345, CAUCHY 2.385, TUKEY 4.685, GEMAN_MCCLURE 1, NONE 1), scale 1, scale_min 1e-3; an
 * unknown kernel gives NONE's */
void rmclhip_robust_params_default(int kernel, rmclhip_robust_params* out);
/* RMCLHIP_ERR_INVALID with a message that names the field: an unknown kernel or scale_mode; a non-finite or non-positive scale (FIXED),
 * tuning or scale_min (MAD) */
rmclhip_status rmclhip_robust_params_check(const rmclhip_robust_params* params);
/* the weight above on the host: the expression the kernels evaluate, compiled with the library's host flags.  c must be > 0 */
float rmclhip_robust_weight_host(int kernel, float c, float r);
/* beside rmclhip_statistics_p2l on caller-owned device views (same stream and scratch owner, synchronous).  weights_out_dev (nullable):
 * n floats, the weight of every element, 0 where masked or gated out.  n == 0: identity statistics, scale = c of an empty set. */
rmclhip_status rmclhip_statistics_p2l_robust(rmclhip_ctx* ctx, const rmclhip_transform* Tpre, const float* dataset_points_xyz_dev,
                                             const uint8_t* dataset_mask_dev, const float* model_points_xyz_dev,
                                             const float* model_normals_xyz_dev, const uint8_t* model_mask_dev, uint32_t n, float max_dist,
                                             const rmclhip_robust_params* params, float* weights_out_dev,
                                             rmclhip_robust_statistics* out);
/* The three operator forms below only READ the last find's correspondences, as rmclhip_rcc_compute_cross_statistics does (max_dist'
 * from convergence_progress); they refuse what it refuses and leave the published moment set, rmclhip_ccs_info and what
 * rmclhip_rcc_compute_cross_statistics returns untouched.  Synchronous. */
rmclhip_status rmclhip_rcc_compute_robust_statistics(rmclhip_rcc* rcc, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                                     const rmclhip_robust_params* params, rmclhip_robust_statistics* out);
/* one weight per correspondence (min(dataset, model) floats) into host memory, or device memory with on_device != 0 */
rmclhip_status rmclhip_rcc_robust_weights(rmclhip_rcc* rcc, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                          const rmclhip_robust_params* params, float* weights_out, int on_device);
/* the scale alone: *c_out, the median (0 in FIXED mode) and the gated-in count m; each pointer may be NULL */
rmclhip_status rmclhip_rcc_residual_scale(rmclhip_rcc* rcc, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                          const rmclhip_robust_params* params, float* c_out, float* median_out, uint32_t* m_out);
/* rmclhip_rcc_correct_once (schedule R) with the weights: one find at Tom * Tbo; in MAD mode the scale is selected once, at the
 * identity pre-transform, and held; then n_iter x { weighted reduction at T_snew_sold, rmclhip_umeyama_transform, T_snew_sold *= U },
 * one launch per iteration, everything on the operator's stream with one synchronisation at the end.  stats_s_out (nullable): the last
 * iteration's statistics, SENSOR frame.  n_iter == 0: identity and identity statistics.  An iteration whose weights sum to zero does
 * not move the pose.  The find rewrites the model buffers and, as every find does, drops the published moment set, which described the
 * old buffers: the next rmclhip_rcc_compute_cross_statistics pays one moment pass (or streams) and returns what it returns after a
 * rmclhip_rcc_find at Tom * Tbo.  rmclhip_ccs_info itself is not touched by the call. */
rmclhip_status rmclhip_rcc_correct_once_robust(rmclhip_rcc* rcc, const rmclhip_transform* Tom, const rmclhip_transform* Tbo, uint32_t n_iter,
                                               double convergence_progress, const rmclhip_robust_params* params,
                                               rmclhip_transform* T_onew_oold_out, rmclhip_robust_statistics* stats_s_out);

/* ---- ROBUST MICP FOR SENSOR RIGS: weighted merge, the rig loop, weighted pose information ---------------------------
 * WEIGHTED MERGE.  rmclhip_cross_statistics_merge with real weights where it has the counts: W = wa + wb in double,
 * w1 = (float)wa / (float)W and w2 = (float)wb / (float)W (float32 divisions), then rmclhip_cross_statistics_merge's expressions,
 * operation for operation.  out.n_meas = a.n_meas + b.n_meas always; W == 0: zero means and covariance, the counts still add;
 * *w_out = W (nullable).  wa or wb negative or non-finite: RMCLHIP_ERR_INVALID.  With wa = a.n_meas and wb = b.n_meas the result is
 * rmclhip_cross_statistics_merge's bytes for every pair of counts whose sum fits 32 bits. */
rmclhip_status rmclhip_cross_statistics_merge_weighted(const rmclhip_cross_statistics* a, double wa, const rmclhip_cross_statistics* b,
                                                       double wb, rmclhip_cross_statistics* out, double* w_out);
/* THE RIG LOOP.  rmclhip_micp_correct_once with the weights, device-resident.  It refuses what rmclhip_micp_correct_once refuses (more
 * than 8 sensors: RMCLHIP_ERR_UNSUPPORTED; sensors of different contexts, a negative or non-finite multiplier) and what
 * rmclhip_robust_params_check refuses; every message names the sensor's index, and every refusal of an argument comes before any
 * launch or change of state (an allocation or HIP error later is returned after every sensor's stream has drained).  params: n_sensors entries, one per sensor -- sensors differ in noise.
 *   - Every sensor gets one plain find at Tom * Tbo[s] on its own stream (no moment epilogue; the moment set is dropped, as by every find).
 *   - Every sensor's scale is its own: in MAD mode selected once behind that sensor's find, at the identity pre-transform, under that
 *     sensor's max_dist' (from convergence_progress), and HELD for all iterations.
 *   - n_iter times: per sensor the weighted statistics at its T_snew_sold (the reduction of rmclhip_rcc_compute_robust_statistics: same
 *     rows, same fold); Cs_o = Tbo * (Tsb * stats_s); `merged` folds the Cs_o with weight_sum_s, `merged_w` with
 *     weight_sum_s * merge_weight_multiplier[s] (NULL: all 1) -- the product is NOT truncated to an integer as the plain loop truncates
 *     n_meas * multiplier (micp_localization.cpp:934): a weight need not be a count.  T_onew_oold *= umeyama(merged_w) when merged_w's
 *     weight is above 0; an iteration without weight moves nothing.  The next pre-transforms are formed as in the plain loop.
 *   - One synchronisation at the end; when the call returns, every sensor's model buffers hold its scan at Tom * Tbo[s].
 * merged_out: `merged` of the last iteration, *merged_weight_out (nullable) its weight; stats_s_out (nullable): n_sensors records, the
 * last iteration's statistics in each SENSOR's frame.  n_iter == 0: identity, identity statistics.  ONE sensor with a multiplier above
 * 0 is rmclhip_rcc_correct_once_robust (the same algebra in the sensor frame, carried to the odometry frame once at the end): its bytes
 * for T and stats_s_out[0]. */
rmclhip_status rmclhip_micp_correct_once_robust(rmclhip_rcc* const* sensors, uint32_t n_sensors, const rmclhip_transform* Tom,
                                                const rmclhip_transform* Tbo, const double* merge_weight_multiplier,
                                                const rmclhip_robust_params* params, uint32_t n_iter, double convergence_progress,
                                                rmclhip_transform* T_onew_oold_out, rmclhip_cross_statistics* merged_out,
                                                double* merged_weight_out, rmclhip_robust_statistics* stats_s_out);
/* WEIGHTED POSE INFORMATION.  rmclhip_rcc_pose_information with the weights the robust loop ends with: info.A = sum w J^T J,
 * info.g = sum w J^T r, info.rss = sum w r^2 (every term (double)w * (u[a] * u[b]), the plain call's grid and fold), info.n_meas the
 * gated-in count; weight_sum = sum w, rss_unweighted = sum r^2.  The scale is selected as rmclhip_rcc_residual_scale selects it at
 * that pre-transform.  The call only reads the last find's buffers: moment set and rmclhip_ccs_info stay untouched.  With NONE, `info`
 * is rmclhip_rcc_pose_information's bytes. */
typedef struct rmclhip_pose_information_robust {
  rmclhip_pose_information info;
  double weight_sum, rss_unweighted;
  float scale, median_abs_residual;
} rmclhip_pose_information_robust;
rmclhip_status rmclhip_rcc_pose_information_robust(rmclhip_rcc* rcc, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                                   const rmclhip_robust_params* params, rmclhip_pose_information_robust* out);
/* rmclhip_pose_covariance_host's algebra on in->info with s2 = info.rss / (weight_sum - 6) when sigma <= 0: the weights' sum stands
 * for the count of effective measurements.  That case is refused unless weight_sum > 6.  weight_sum == n_meas gives
 * rmclhip_pose_covariance_host's bytes. */
rmclhip_status rmclhip_pose_covariance_robust_host(const rmclhip_pose_information_robust* in, const rmclhip_pose_covariance_params* p,
                                                   rmclhip_pose_covariance* out);

/* ---- DISTANCE FIELD: the closest-point sensor update by lookup ----------------------------------------------------
 * sensor_update.correspondence_type 1 (evaluate_cpc) scores a beam by the distance of its end point to the surface: the likelihood
 * is smooth in the pose, without the grazing-ray cliffs of ray casting -- what AMCL users know as the likelihood-field model, and the
 * mode a global localisation wants.  The map is immutable, so that distance can be tabulated once: a distance field is a regular
 * lattice of float32 distances to the closest triangle, built on the device from a map.  With a field attached (rmclhip_pf_set_field)
 * the sensor update answers correspondence_type 1 from the lattice -- eight loads and a trilinear blend per beam, no tree.  A handle
 * without a field returns the bytes it returned before this interface existed.
 *
 * THE GEOMETRY.  Every operation is in float32 unless it says double; the library is built without contraction
 * (tests/field_ref.py restates this in numpy).
 *   - Per axis k: ext_k = (bbox_max_k - bbox_min_k) + 2 * margin and origin_k = bbox_min_k - margin.
 *   - Automatic cell (params.cell == 0): cell = float(cbrt(max(ext_x, 1e-3) * max(ext_y, 1e-3) * max(ext_z, 1e-3) / 2e6)), in double.
 *     This is the near grid's size rule.
 *   - n_k = max(2, uint(ceil(ext_k / cell)) + 1) nodes.
 *   - inv_cell = 1.0f / cell.
 *   - Node (i, j, k) lies at origin + (float(i) * cell, float(j) * cell, float(k) * cell), product first, then sum.
 *   - Node value: the distance the library's own closest-point query reports for that point: sqrtf(d2) of the query of
 *     rmclhip_rcc_find_cpc / correspondence_type 1 (smallest d2, then smallest face id).  A node whose query finds nothing stores NaN.
 *   The build runs coarse to fine: every 16th node per axis first, then every 4th, then all, each level's queries starting from the
 *   triangle the level before found for the nearest node -- an actual candidate, so the values are those of unseeded queries, and the
 *   same map and parameters give the same bytes on every device.
 *
 * THE LOOKUP at a point P (map coordinates).
 *   - If any component of P fails |P_k| <= FLT_MAX, the result is NaN.
 *   - u_k = (P_k - origin_k) * inv_cell.
 *   - c_k = min(max(u_k, 0), float(n_k - 1)).
 *   - i_k = min(int(floor(c_k)), n_k - 2).
 *   - f_k = c_k - float(i_k).
 *   - lerp(a, b, f) = a + f * (b - a).  Lerp four times along x, twice along y, once along z.  Call the result d.
 *   - Axis k is clamped when u_k < 0 or u_k > float(n_k - 1).  o_k = P_k - (origin_k + c_k * cell) on clamped axes, and 0 on the others.
 *     If any axis is clamped, the result is d + sqrtf((o_x^2 + o_y^2) + o_z^2).  Otherwise it is d.
 *
 * WHAT THIS GUARANTEES.  The distance d(P) to the surface is 1-Lipschitz, and the blend's weights w_c over the cell's corners c
 * satisfy sum_c w_c |c - P| <= sqrt(sum_k cell^2 f_k (1 - f_k)) <= (sqrt(3) / 2) cell.
 *   - Inside the lattice, |lookup - d(P)| <= (sqrt(3) / 2) * cell plus rounding.
 *   - Outside, the lookup never reports less than d(P) - (sqrt(3) / 2) * cell.  It may report up to twice the distance to the box more. */
typedef struct {
  float cell;          /* node spacing in metres; 0 (the default): automatic */
  float margin;        /* the lattice extends this far beyond the map's box on every side; default 0 */
  uint64_t max_nodes;  /* a lattice of more nodes is refused; default 2^26 (256 MiB) */
} rmclhip_field_params;
void rmclhip_field_params_default(rmclhip_field_params* out);
typedef struct {
  uint32_t n[3];       /* nodes per axis */
  float origin[3];     /* node (0, 0, 0) */
  float cell, inv_cell;
  uint64_t n_nodes, bytes;
} rmclhip_field_info;
/* host only, no device needed: the geometry rmclhip_field_create will use for a map with this box.  RMCLHIP_ERR_INVALID: cell or margin
 * negative or not finite, a box that is not finite or has min > max, a lattice of more than max_nodes nodes.  params NULL: the defaults */
rmclhip_status rmclhip_field_layout_host(const float bbox_min[3], const float bbox_max[3], const rmclhip_field_params* params,
                                         rmclhip_field_info* info_out);
/* builds the field of `map` on its device and waits for it.  The field retains the map and is immutable; its bytes are added to the
 * map's device_bytes (rmclhip_map_get_info) while it lives.  Refused with RMCLHIP_ERR_INVALID before anything is launched: what
 * rmclhip_field_layout_host refuses, and a map with no faces.  rmclhip_field_destroy drops the creator's reference: a filter handle
 * the field is set on keeps it alive */
rmclhip_status rmclhip_field_create(rmclhip_ctx* ctx, rmclhip_map* map, const rmclhip_field_params* params, rmclhip_field** out);
void rmclhip_field_destroy(rmclhip_field* field);
rmclhip_status rmclhip_field_get_info(const rmclhip_field* field, rmclhip_field_info* out);
/* the node values to host memory, x fastest, then y, then z; capacity: floats `out` has room for (>= n_nodes) */
rmclhip_status rmclhip_field_download(rmclhip_field* field, float* out, size_t capacity);
/* the lattice in device memory, in rmclhip_field_download's order; valid while the field lives, read only */
rmclhip_status rmclhip_field_device_view(const rmclhip_field* field, const float** lattice_dev);
/* the lookup alone for n points (xyz triples, map coordinates).  points_on_device != 0: points_xyz and distances_out are device
 * memory of the field's device; else host memory.  n == 0: RMCLHIP_OK, nothing is touched; null pointers with n > 0: RMCLHIP_ERR_INVALID */
rmclhip_status rmclhip_field_query(rmclhip_field* field, const float* points_xyz, size_t n, int points_on_device, float* distances_out);
/* later rmclhip_pf_update[_async] calls on this handle answer correspondence_type 1 from the field: per (particle, beam) the end point
 * Tsm * orig + (Tsm.R * dir) * range exactly as without a field, the error is the lookup there (a NaN error poisons the particle, as it
 * does without a field), evaluated and merged in beam order as correspondence_type 1 is -- the in-order chain, bit for bit for the
 * same errors; n_meas is exact.  rmclhip_pf_set_error_output works as in every other mode; rmclhip_pf_set_mapping / _set_variant are
 * not read (one dealing, results do not depend on it).  NULL switches it off; a fresh handle has it off.  The handle keeps a reference
 * to the field.  RMCLHIP_ERR_INVALID if the field is of another map.  While a field is set and correspondence_type != 1,
 * rmclhip_pf_update[_async] return RMCLHIP_ERR_INVALID and touch nothing */
rmclhip_status rmclhip_pf_set_field(rmclhip_pf* pf, rmclhip_field* field);
/* every replica builds its own field from its own copy of the map (the build is deterministic: all replicas hold the same bytes) and
 * sets it on its filter handle, replacing an earlier one; NULL switches it off */
rmclhip_status rmclhip_pf_sharded_set_field(rmclhip_pf_sharded* pf, const rmclhip_field_params* params);

/* ---- BANDED DISTANCE FIELD: fine cells on large maps, stored near the surface ----------------------------------------
 * A dense lattice at a fine cell does not fit a large map, and most of it is never needed at full resolution: beyond a few sigma the
 * sensor update's exp(-d^2 / 2 sigma^2) is 0 whatever d's third digit is, and REFINE / STEIN ignore a beam with d >= max_dist.  A
 * banded field keeps the dense field's geometry and lookup rule, stores fine nodes only in bricks near the surface, and answers the
 * rest from a coarse lattice.  The handle is an rmclhip_field: rmclhip_field_query, rmclhip_pf_set_field, rmclhip_pf_update[_async],
 * rmclhip_field_refine, rmclhip_pf_refine, rmclhip_pf_stein_step, rmclhip_field_get_info (the logical geometry, the actual bytes) and
 * the map's device_bytes work on it unchanged.  rmclhip_field_download and rmclhip_field_device_view return RMCLHIP_ERR_INVALID on it.
 *
 * THE LAYOUT (tests/band_field_ref.py restates this in numpy).
 *   - Logical lattice: exactly the dense field's origin, cell, inv_cell and n_k (THE GEOMETRY above; an automatic cell is the dense
 *     rule), without the cap on the node count.  n_k - 1 <= 2^20 on every axis.
 *   - Bricks: a brick is 8 cells per axis, nb_k = ceil((n_k - 1) / 8).  Brick (bx, by, bz) owns the logical nodes 8 b_k ... 8 b_k + 8 on
 *     each axis: 9^3 = 729 floats, the shared faces duplicated, so the eight corners of any cell come from one brick.  In-brick order
 *     is x fastest: node (lx, ly, lz) at (lz * 9 + ly) * 9 + lx.  Nodes of a ragged last brick beyond n_k - 1 hold NaN and are never
 *     read (i_k <= n_k - 2).
 *   - Coarse lattice: dense, nb_k + 1 nodes per axis, x fastest.  Coarse node c_k holds the field's value at logical node
 *     min(8 c_k, n_k - 1): the dense node value, i.e. the library's own closest-point query there.
 *   - Classification: reach = band + 6.9282032f * cell in float (band + 4 sqrt(3) cell: no point of a brick is farther than
 *     4 sqrt(3) cell from its nearest corner).  A brick is STORED iff the minimum of its eight coarse corner values is <= reach, or a
 *     corner is NaN.  Otherwise it is FAR.
 *   - Stored bricks are numbered by an exact prefix scan in brick order (x fastest): stored index = the number of stored bricks before
 *     it.  The numbering never follows an arrival order, so every device builds the same bytes.  A uint32 table, one word per brick
 *     in brick order, holds the stored index or 0xFFFFFFFF (FAR).
 *   - Fine nodes of stored bricks hold the dense field's node values (a build seed is only a candidate; the value is the unseeded
 *     query's).
 *
 * THE LOOKUP.  The finite check, u_k, c_k, i_k, f_k, the clamped axes and o_k are THE LOOKUP's above.  The cell's brick is b_k = i_k >> 3.
 *   - STORED brick: the eight corners are read from the brick at local index i_k & 7; the blend and the clamp term are unchanged.  The
 *     result is the dense field's, to the bit.
 *   - FAR brick: the cell is the brick.  The eight corners are the brick's coarse corners and the fractions are
 *     F_k = (c_k - float(8 b_k)) / float(e_k) with e_k = min(8, (n_k - 1) - 8 b_k); the same blend, the same clamp term.  Every corner
 *     exceeds reach, so the result exceeds band -- and, d being 1-Lipschitz, so does the true distance.  The error is bounded by
 *     (sqrt(3) / 2) * 8 * cell plus rounding.
 *   - The value-with-gradient lookup of REFINE ON THE FIELD: a beam whose cell lies in a FAR brick is NOT VALID, the rule a clamped
 *     axis already follows.
 *
 * CONSEQUENCES.  With max_dist <= band, rmclhip_field_refine, rmclhip_pf_refine, rmclhip_pf_sharded_refine and rmclhip_pf_stein_step on
 * a banded field give the dense field's bytes: a beam in a FAR brick has d > band >= max_dist on the dense field, and is not used
 * there either (an unused beam adds max_dist^2 to the cost whether or not it is valid).  max_dist > band on a banded field is refused
 * with RMCLHIP_ERR_INVALID before anything is launched. */
typedef struct {
  float cell;          /* node spacing in metres; 0 (the default): automatic, the dense field's rule */
  float margin;        /* as rmclhip_field_params; default 0 */
  uint64_t max_nodes;  /* counts STORED nodes: 729 * n_stored + n_coarse beyond it is refused; default 2^26 (256 MiB) */
  float band;          /* fine values are kept wherever the distance may be <= band; default 0.5, > 0 and finite */
  uint32_t reserved;   /* 0 */
} rmclhip_band_field_params;
void rmclhip_band_field_params_default(rmclhip_band_field_params* out);
typedef struct {
  uint32_t nb[3];      /* bricks per axis */
  uint32_t brick_edge; /* 8 */
  uint64_t n_bricks, n_stored, n_coarse;
  float band, reach;
  uint64_t bytes;      /* table + coarse lattice + stored bricks, as held on the device */
} rmclhip_band_field_info;
/* host only, no device needed: the logical geometry and the bricks rmclhip_field_create_banded will use for a map with this box;
 * n_stored and both bytes are 0 (they depend on the map).  RMCLHIP_ERR_INVALID: what rmclhip_field_layout_host refuses except the node
 * count, band not positive and finite, more than 2^20 cells on an axis, a coarse lattice of more than max_nodes nodes */
rmclhip_status rmclhip_band_field_layout_host(const float bbox_min[3], const float bbox_max[3], const rmclhip_band_field_params* params,
                                              rmclhip_field_info* logical_out, rmclhip_band_field_info* info_out);
/* builds the banded field of `map` on its device and waits for it: the coarse lattice by seeded queries (every 16th logical node, then
 * every 8th), the classification, the exact scan, one count read back, then the stored bricks.  Refused with RMCLHIP_ERR_INVALID: what
 * rmclhip_band_field_layout_host refuses and a map with no faces before anything is launched; 729 * n_stored + n_coarse > max_nodes
 * once the count is known -- everything allocated is freed and the map's device_bytes is what it was.  Lifetime and accounting are
 * rmclhip_field_create's */
rmclhip_status rmclhip_field_create_banded(rmclhip_ctx* ctx, rmclhip_map* map, const rmclhip_band_field_params* params, rmclhip_field** out);
/* RMCLHIP_ERR_INVALID on a dense field */
rmclhip_status rmclhip_field_get_band_info(const rmclhip_field* field, rmclhip_band_field_info* out);
/* the three arrays to host memory: table (n_bricks words), coarse (n_coarse floats), bricks (729 * n_stored floats, in stored order).
 * Each pointer may be NULL (that array is skipped); each capacity counts elements.  RMCLHIP_ERR_INVALID on a dense field */
rmclhip_status rmclhip_field_download_banded(rmclhip_field* field, uint32_t* table, size_t table_capacity, float* coarse, size_t coarse_capacity,
                                             float* bricks, size_t bricks_capacity);
/* rmclhip_pf_sharded_set_field with a banded field on every replica (same bytes on all); NULL switches the field off */
rmclhip_status rmclhip_pf_sharded_set_field_banded(rmclhip_pf_sharded* pf, const rmclhip_band_field_params* params);

/* ---- REFINE ON THE FIELD: damped Gauss-Newton of every particle by lookup -------------------------------------------
 * The eight lattice values that give the distance at a beam's end point also give its gradient, so a particle can be moved towards the
 * map, not only weighed against it: a per-particle Levenberg-Marquardt refinement of the cost sum_b min(d_b, max_dist)^2, all
 * iterations inside one launch, no tree, no stack.  Likelihood attributes are NEVER touched: a refined pose has not been scored, the
 * caller follows with a sensor update.  (This is the gradient half of a Stein variational step; the neighbours' average and the
 * repulsion between particles are STEIN STEP ON THE FIELD, below.)
 *
 * THE ARITHMETIC.  Everything is float32 unless it says double; the library is built without contraction and the device evaluates no
 * transcendental (tests/refine_ref.py restates this in numpy; the device matches it byte for byte).
 *   Per beam b of a particle with pose (R, t):  Tsm = pose * Tsb, the end point M = Tsm * orig + (Tsm.R * dir) * range exactly as the
 *   field's sensor update forms it, and the lever L = M - t, componentwise.
 *   Lookup with gradient at M: index, fraction and clamping are THE LOOKUP's; d is its value, bit for bit.  With the eight corner
 *   values v_xyz of the cell, (fx, fy, fz) its fractions and lerp(a, b, f) = a + f * (b - a):
 *     gx = lerp(lerp(v100 - v000, v110 - v010, fy), lerp(v101 - v001, v111 - v011, fy), fz) * inv_cell
 *     gy = lerp(lerp(v010 - v000, v110 - v100, fx), lerp(v011 - v001, v111 - v101, fx), fz) * inv_cell
 *     gz = lerp(lerp(v001 - v000, v101 - v100, fx), lerp(v011 - v010, v111 - v110, fx), fy) * inv_cell
 *   The gradient is not normalised.  A beam is VALID when every component of M passes |M_k| <= FLT_MAX, no axis is clamped (M lies
 *   inside the lattice) and d, gx, gy, gz are finite (no NaN corner).  A beam is USED when it is valid and d < max_dist.
 *   Cost of a pose: C = sum_b rho_b in double, rho_b = double(m) * double(m) with m = d for a used beam and max_dist for any other
 *   (that is min(d, max_dist)^2 for a valid beam).
 *   Normal equations over the used beams, for the perturbation M' ~ M + v + omega x L (a translation v and a world-axes rotation omega
 *   about the particle's own position): J = (gx, gy, gz, Ly*gz - Lz*gy, Lz*gx - Lx*gz, Lx*gy - Ly*gx) in float, unfused; r = d.  In
 *   double: the 21 entries A_ij += double(J_i) * double(J_j) (i <= j), the 6 entries b_i += double(J_i) * double(r), and the count n_used.
 *   Summation order (C, A, b alike): 64 partial sums; partial l takes the beams l, l + 64, l + 128, ... in increasing order, starting
 *   from +0; then six rounds s = 32, 16, 8, 4, 2, 1 in which every partial l becomes partial_l + partial_(l xor s); the total is
 *   partial 0.  It does not depend on the launch, on the number of particles or on sharding.
 *   Step, in double: a degree of freedom k whose bit in dof_mask is clear (bits 0..5: x, y, z, rotation about world x, y, z) gets row
 *   and column k of A set to 0, A_kk = 1, b_k = 0.  H = A with H_kk = (A_kk + lambda * A_kk) + 1e-9.  H = G G^T by Cholesky without
 *   pivoting, column by column: s = H_jj - G_j0^2 - ... - G_j,j-1^2 (subtracted one by one), G_jj = sqrt(s), G_ij = (H_ij - G_i0 G_j0 -
 *   ... ) / G_jj; a pivot s that is not > 0 REJECTS the step.  G y = b forwards, G^T x = y backwards (terms subtracted in increasing
 *   index, then one division), delta = -x, and 0 for a locked k.  |v| = sqrt((v_x^2 + v_y^2) + v_z^2), |omega| alike; the whole delta is
 *   multiplied by the smallest of 1, max_step_trans / |v| (if |v| > 0) and max_step_rot / |omega| (if |omega| > 0).
 *   Candidate pose: t'_k = t_k + float(v_k) on the free translation axes (a locked one is copied); if any rotation is free,
 *   q' = normalise((float(0.5 * omega), w = 1) * R) with the quaternion product and the four-division normalise of the surface
 *   constraint (else R is copied).  First order, which suffices: the fixed point is delta = 0.
 *   Loop: one pass computes (C, A, b, n_used) at a pose.  The start pose is evaluated; then `iterations` times: solve; if not rejected
 *   evaluate the candidate; if C_cand < C_cur the candidate becomes the current pose with its A, b and n_used and
 *   lambda = max(lambda / 3, 1e-6); otherwise (rejected, or no smaller cost) lambda = lambda * 10.  lambda starts at double(lambda0).
 *   By construction cost_after <= cost_before for every particle.
 *   Untouched, bit for bit: iterations == 0, dof_mask == 0, n_used == 0 at the start, a pose with a component that is not finite, and
 *   every particle that accepted no step.  A result row is written in each of these cases too. */
typedef struct {
  uint32_t iterations;     /* default 8, at most 64 */
  uint32_t dof_mask;       /* default 0x3F; bits 0..5: x, y, z, rotation about world x, y, z; at most 0x3F */
  float max_dist;          /* default 0.5, must be > 0: a beam farther from the surface is not used and costs max_dist^2 */
  float max_step_trans;    /* default 0.5 (metres per iteration), must be > 0 */
  float max_step_rot;      /* default 0.25 (radians per iteration), must be > 0 */
  float lambda0;           /* default 1e-3, must be > 0 */
} rmclhip_refine_params;
void rmclhip_refine_params_default(rmclhip_refine_params* out);
typedef struct {
  float cost_before, cost_after;   /* float(C) at the start pose and at the final pose */
  uint32_t n_used;                 /* at the final pose */
  uint32_t accepted;               /* steps */
} rmclhip_refine_result;
typedef struct {
  uint32_t n_particles;
  uint32_t n_moved;        /* accepted at least one step */
  uint32_t n_no_beams;     /* finite pose, n_used == 0 at the start */
  uint32_t n_not_finite;   /* a pose component is not finite */
  double cost_before_sum, cost_after_sum;   /* the rows' costs summed in double in particle order */
} rmclhip_refine_stats;
/* refines n_particles poses (device memory of the field's device) in place and waits for it.  beams: host memory, n_beams records, at
 * most 8192 (the field sensor update's bound); Tsb as in rmclhip_pf_update; params NULL: the defaults.  results_dev (nullable): device
 * memory for one row per particle; stats_out (nullable).  n_particles == 0: RMCLHIP_OK, nothing is touched.  RMCLHIP_ERR_INVALID before
 * anything is launched: a parameter that is not finite or outside its range, null poses / beams / Tsb with n_particles > 0, n_beams 0
 * or above 8192 */
rmclhip_status rmclhip_field_refine(rmclhip_field* field, rmclhip_transform* poses_dev, uint32_t n_particles,
                                    const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                    const rmclhip_refine_params* params, rmclhip_refine_result* results_dev, rmclhip_refine_stats* stats_out);
/* the same on the field set with rmclhip_pf_set_field, on the handle's stream (behind whatever was enqueued on it); the same bytes.
 * RMCLHIP_ERR_INVALID when no field is set */
rmclhip_status rmclhip_pf_refine(rmclhip_pf* pf, rmclhip_transform* poses_dev, uint32_t n_particles, const rmclhip_range_measurement* beams,
                                 uint32_t n_beams, const rmclhip_transform* Tsb, const rmclhip_refine_params* params,
                                 rmclhip_refine_result* results_dev, rmclhip_refine_stats* stats_out);
/* every replica refines its own block on its own field (rmclhip_pf_sharded_set_field), no collective: particles are independent, so
 * the poses equal the unsharded call's bit for bit.  stats_out: the replicas' counts and sums added in rank order */
rmclhip_status rmclhip_pf_sharded_refine(rmclhip_pf_sharded* pf, const rmclhip_range_measurement* beams, uint32_t n_beams,
                                         const rmclhip_transform* Tsb, const rmclhip_refine_params* params, rmclhip_refine_stats* stats_out);

/* ---- STEIN STEP ON THE FIELD: neighbour-averaged moves and repulsion ---------------------------------------------------
 * REFINE ON THE FIELD moves every particle on its own, and eight iterations put every particle of a basin on one point.  A Stein
 * variational step moves particle i by the kernel-weighted average of its neighbours' moves and pushes it away from them, so the cloud
 * goes down the cost and keeps a width.  One call runs `iterations` such steps on the handle's stream, with no host round trip between
 * their phases.  Likelihood attributes are NEVER touched: the caller follows with a sensor update.
 *
 * THE ARITHMETIC (tests/stein_ref.py restates it in numpy; the device matches it byte for byte).  float32 and unfused unless it says
 * double.  Iteration `it` = 0 .. iterations - 1; every neighbour term is computed from the poses as they were at the iteration's start.
 *   1. Drive.  For a particle j with a finite pose: one pass of REFINE ON THE FIELD at its pose (C, A, b, n_used) and one solve at
 *      lambda = double(lambda0), the step limits included: refine's first candidate step delta.  drive_j[k] = float(delta_k); the drive
 *      is zero when n_used == 0, when the solve is rejected and on locked degrees of freedom.  A particle with a pose component that is
 *      not finite is untouched, has no drive and is nobody's neighbour.
 *   2. Cell list over the FREE translation axes.  width = 1.001f * h_trans; the bin of t_k on a free axis is the translation bin of BINS
 *      (floor(t_k / width) clamped to -8192 .. 8191), a locked axis is ignored; rotations are not binned.  count_B = the finite-pose
 *      particles of bin B.  Every particle of a bin with count_B <= max_per_bin is LISTED; in a fuller bin particle j is listed iff
 *      uint64(r_j) * count_B < uint64(max_per_bin) << 32, r_j = word 0 of draw 8 of the resamplers' random stream, counter
 *      (j, step + it, 8, 0) under the key `seed`.  w_B = float(count_B) / float(listed_B); a bin with listed_B == 0 gives nothing.  The
 *      listed set is a function of indices and counts, never of an arrival order.
 *   3. Pair sums of a particle i with a finite pose.  Candidates: the listed particles j != i of the 3^d bins around i's bin, d = the
 *      number of free translation axes; a bin index beyond the clamp's range does not exist (no wrap).  Since width > h_trans, these
 *      bins hold every j inside the kernel's support.  Per candidate:
 *        e_k = (t_j - t_i)_k / h_trans on the free translation axes;
 *        on the free rotation axes e_k = rho_k / h_rot, rho = 2 * vec(q_j * conj(q_i)) (the Hamilton product of the transform algebra,
 *        conj negates x, y, z), negated if the product's w < 0: world axes, first order -- the convention of refine's omega;
 *        s = the sum of e_k * e_k over the free degrees of freedom in bit order, from +0;
 *        the pair COUNTS iff s < 1; then u = 1 - s, kk = u * u, a = w_B * kk.
 *      The kernel is (1 - s)^2 for s < 1 and 0 beyond: compact support, so the adjacent bins are all of it, and no transcendental.  (It
 *      is chosen for support and exactness, not for positive definiteness.)  With Q(x) = int64(rint(double(x) * 2^32)):
 *        W += Q(a);   D_k += Q(a * drive_j[k]);   R_k += Q((w_B * u) * e_k)   on the free degrees of freedom k;
 *        the self term: W += 2^32, D_k += Q(drive_i[k]).
 *      The sums are 64-bit integers: exact in any order, so the result does not depend on the order inside a bin, on the launch or on
 *      the schedule.  (sum of a <= n_particles <= 2^26, |drive| <= 16, |e_k| < 1: every |sum| < 2^63.)
 *   4. Move, in double: phi_k = (double(D_k) - ((double(repulsion) * 4) * double(h_k)) * double(R_k)) / double(W), h_k = h_trans for
 *      k < 3 and h_rot else; 0 on a locked degree of freedom.  (-4 u e_k / h_k is the kernel's gradient with respect to x_j; scaled by
 *      repulsion * h_k^2 both terms are lengths.)  phi is limited in length as refine limits delta and applied by refine's candidate
 *      rule.  There is NO accept test: repulsion is meant to raise a particle's own cost.
 * Not built: the sharded filter (it would need an all-gather of poses and drives). */
typedef struct {
  uint32_t iterations;     /* default 1, at most 64 */
  uint32_t dof_mask;       /* default 0x3F: refine's bits */
  float max_dist;          /* default 0.5, must be > 0: as in refine */
  float max_step_trans;    /* default 0.5, must be > 0 and <= 16 */
  float max_step_rot;      /* default 0.25, must be > 0 and <= 16 */
  float lambda0;           /* default 1e-3, must be > 0 */
  float h_trans;           /* default 0.25 (metres): the kernel's bandwidth in translation, must be > 0 */
  float h_rot;             /* default 0.2 (radians): ... in rotation, must be > 0 */
  float repulsion;         /* default 0.25, must be >= 0 and finite; 0: the kernel-weighted average alone */
  uint32_t max_per_bin;    /* default 256, must be >= 1: fuller bins are thinned to about this many listed particles */
  uint64_t seed;           /* default 0: the key of the thinning's random stream */
  uint32_t step;           /* default 0: its step; iteration `it` uses step + it */
} rmclhip_stein_params;
void rmclhip_stein_params_default(rmclhip_stein_params* out);
typedef struct {
  float cost;              /* float(C) at the pose the LAST iteration started from */
  uint32_t n_used;         /* at that pose */
  uint32_t n_neighbours;   /* the pairs with s < 1 in the last iteration */
  float kernel_weight;     /* float(double(W) * 2^-32) of the last iteration; 0 for a pose that is not finite */
} rmclhip_stein_result;
typedef struct {
  uint32_t n_particles;
  uint32_t n_not_finite;   /* a pose component is not finite */
  uint32_t n_no_beams;     /* finite pose, n_used == 0 */
  uint32_t n_bins;         /* occupied bins of the cell list */
  uint32_t n_thinned_bins; /* bins with count_B > max_per_bin; all four from the last iteration */
  uint32_t reserved;
  double cost_sum;         /* the rows' costs summed in double in particle order */
} rmclhip_stein_stats;
/* runs `iterations` Stein steps on n_particles poses (device memory) in place, on the field set with rmclhip_pf_set_field, on the
 * handle's stream, and waits for them.  beams, n_beams, Tsb, params NULL, results_dev, stats_out: as in rmclhip_pf_refine.  The scratch
 * belongs to the handle: it only grows and is freed with it.  n_particles == 0: RMCLHIP_OK, nothing is touched; iterations == 0:
 * RMCLHIP_OK, nothing is launched and no row is written.  RMCLHIP_ERR_INVALID before anything is launched: a parameter outside its
 * rule, n_particles > 2^26, no field set, and everything rmclhip_pf_refine refuses */
rmclhip_status rmclhip_pf_stein_step(rmclhip_pf* pf, rmclhip_transform* poses_dev, uint32_t n_particles, const rmclhip_range_measurement* beams,
                                     uint32_t n_beams, const rmclhip_transform* Tsb, const rmclhip_stein_params* params,
                                     rmclhip_stein_result* results_dev, rmclhip_stein_stats* stats_out);

/* ---- device memory helpers for hosts without their own allocator ---------------------- */
rmclhip_status rmclhip_malloc(rmclhip_ctx* ctx, size_t bytes, void** out_dev);
rmclhip_status rmclhip_free(rmclhip_ctx* ctx, void* ptr_dev);
rmclhip_status rmclhip_memcpy_h2d(rmclhip_ctx* ctx, void* dst_dev, const void* src, size_t bytes);
rmclhip_status rmclhip_memcpy_d2h(rmclhip_ctx* ctx, void* dst, const void* src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* RMCLHIP_H */
