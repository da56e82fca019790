/* rmclhip_lab.h -- EXPERIMENTS of librmclhip (librmclhip_lab.so): measured-and-rejected kernel variants and in-kernel
 * instrumentation, kept buildable for A/B runs (tools/) and for the `lab` group of the GPU tests.  NOT part of the drop-in
 * boundary: nothing here replaces a reference interface, and a product build never needs this header or that library.
 *
 * Loading librmclhip_lab.so (dlopen / ctypes.CDLL, after librmclhip.so) registers its launchers with the product; from then on
 *   rmclhip_rcc_set_variant accepts the traversal kinds
 *       1  one lane per ray, branch-free step                 4  one lane per ray on the 64-B quantised nodes
 *       5  while-while step, tails of every wave finished by quads
 *       6 / 7   kind 5 + the top 85 / 341 nodes resident in LDS (north_star "LDS-staged node tiles"; flat loads)
 *       8       kind 5 + one-round-trip leaves                 9 / 10  kind 8 + the LDS top
 *       11 the round-1 branchy step                            12 branch-free step + one-round-trip leaves
 *       13 / 14 wave-uniform nodes through the scalar cache ("wavefront ballot"; 14: + one-round-trip leaves)
 *       16 / 17 branch-free step + quad-finished tails (17: + one-round-trip leaves)      20 kind 16 + the leaf trigger
 *       19 / 21 / 22  round 2's automatic choices (17 / 5 / 4 with the leaf trigger), superseded by 23 / 24 = 19 / 22 + frontier start
 *       25 kind 2 (four lanes per ray) + frontier start        26 kind 23 on the 64-B quantised nodes
 *       27 kind 23 + prefetch of the hit record's normal / face id during the traversal
 *       28 kind 23 with a software-pipelined node step (next node requested after three of the five ordering steps, top of the stack in a register)
 *       29 / 30 kind 23 with four / three of the five ordering steps of a node's children    (round 3: 25 ... 30 measured, not adopted)
 *     (spherical model only; results are bit-identical to the product's kinds, tests/test_gpu_lab.py), and
 *   rmclhip_pf_set_variant accepts the round kernels (bits 4..6 = 0) and the round-2 persistent kernel (bits 7 / 8).
 * Measurements of every kind: profiles/r02_find_variants_ab.txt, profiles/r03_find_variants_ab.txt, DESIGN.md 4. */
#ifndef RMCLHIP_LAB_H
#define RMCLHIP_LAB_H

#include "rmclhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* exported by librmclhip_lab.so */
const char* rmclhip_lab_version(void);

/* The two entry points below are exported by librmclhip.so (they need the handle's internals) but work only while
 * librmclhip_lab.so is loaded -- the instrumented kernels live there; RMCLHIP_ERR_UNSUPPORTED otherwise. */

/* TEST output of the surface constraint (rmclhip.h: rmclhip_pf_set_surface / rmclhip_pf_constrain_to_surface): while faces_dev is set
 * (borrowed device memory, one word per particle of the largest call; NULL switches it off) every constrained launch on the handle
 * also stores the ORIGINAL id of the face each particle's probe hit, 0xFFFFFFFF for none -- what tests/test_gpu_surface.py holds
 * against the brute-force oracle where the ray runs along shared edges.  Works without the experiments library. */
rmclhip_status rmclhip_debug_surface_faces(rmclhip_pf* pf, uint32_t* faces_dev);
/* tools/wave_timeline.py: one spherical find() of the current variant whose waves record their entry / exit shader clock:
 * out = n_waves x 8 dwords {s_memtime entry, exit (stores completed), s_memrealtime entry (100 MHz), tile | xcc << 24,
 * s_memtime before the traversal, after it, stores issued, 0} (all zero = wave had no tile) */
rmclhip_status rmclhip_debug_wave_clock(rmclhip_rcc* rcc, const rmclhip_transform* Tbm_est, uint32_t* out, size_t cap_dwords,
                                        uint32_t* n_waves_out);
/* TEST read-out of the one table of find traversal kinds and of the launch shape every launcher derives from it
 * (tests/test_find_kinds_cpu.py): what a find of `kind` over tiles_x x tiles_y tiles and nposes poses would be launched with -- with the
 * MICP moment epilogue when `moments` != 0 and the kind has one, over a world order of n_tile_order entries (0: pose-major) dealt
 * `granule` workgroups per XCD turn.  Pure arithmetic: touches no device and no handle; works without the experiments library.  A
 * number that is no kind: exists = 0 and every other field 0. */
typedef struct rmclhip_find_launch_shape {
  uint32_t exists, in_product;   /* a kind at all; built into librmclhip.so */
  uint32_t tiles_per_block;      /* 64-ray tiles per workgroup = mask words per workgroup of the epilogue = group of the world order */
  uint32_t grid_x, grid_y;       /* blocks of 256 threads */
  uint32_t lds_bytes;            /* dynamic LDS per workgroup */
  uint32_t clock_dwords;         /* what a clocked launch (rmclhip_debug_wave_clock) writes */
  uint32_t has_moments;          /* the kind has the moment epilogue */
} rmclhip_find_launch_shape;
rmclhip_status rmclhip_debug_find_launch_shape(int kind, int moments, uint32_t tiles_x, uint32_t tiles_y, uint32_t nposes,
                                               uint32_t n_tile_order, uint32_t granule, rmclhip_find_launch_shape* out);
/* the moments the LAST moment-form attempt of rmclhip_rcc_correct_once worked from (rmclhip.h: rmclhip_rcc_set_micp_fast): the 96 sums
 * of its partial rows (82 used; layout in reduce_common.hip.h) and the number of correspondences it left undecided.  Works without the
 * experiments library. */
rmclhip_status rmclhip_debug_micp_moments(rmclhip_rcc* rcc, double* totals96, uint32_t* n_rows_out, uint64_t* n_uncertain_out);
/* tools/probe_find.py: one spherical find() through an instrumented copy of the one-lane-per-ray traversal that stamps
 * s_memtime around every node / leaf step of every wave.  mode: bit 0 = one-round-trip leaves, bit 1 = LDS-resident top of the
 * tree.  log_out: n_tiles x 512 dwords (host). */
rmclhip_status rmclhip_debug_probe_find(rmclhip_rcc* rcc, const rmclhip_transform* Tbm_est, int mode, uint32_t* log_out,
                                        size_t log_cap_dwords, uint32_t* n_tiles_out);

/* A/B knobs of the cooperative descent of find kinds 32 / 31 (traverse.hip.h frontier_descent_start): the wave stops descending when a
 * level would leave more than final_cap entries (<= 64, default 64) or after (max_levels & 255) levels (default 24; 0 = kind 23's
 * frontier start with the descent's bookkeeping); bits 8..15 of max_levels, when not 0: kind 32's bound on the final leaves one ray may
 * enter before its wave starts at the root instead (default 24); bits 29..30, when not 0: 1 + the tile mapping of single scans (0 as
 * dealt, 1 an eighth of the image per XCD, 2 a CU's two workgroups from the image's halves; find_kernel.hip.h) instead of the tuned /
 * default one; bit 16 set: kind 32 keeps accepted candidates undivided through its cooperative leaf loop (rmclhip_rcc_autotune sets it
 * where it measures faster; every call of this function sets or clears it); bit 31 set: descend on the four-wide nodes even where the map carries the 16-wide twins (A/B).  Results do not depend on any of them.  Exported by librmclhip.so. */
rmclhip_status rmclhip_rcc_set_descent(rmclhip_rcc* rcc, uint32_t final_cap, uint32_t max_levels);

/* A/B knob (round 6, VERDICT r5 #7b): pose batches in WORLD ORDER (the default; on = 0 restores the pose-major launch).  Every batch launch
 * (find_batch, correct_batch, simulate with several poses, the sharded forms) of this operator makes one
 * key per workgroup of the launch (four neighbouring tiles of one pose; Morton code of the point where their central ray leaves the map's
 * bounding box), sorts the
 * tiles by key (counting sort over 4096 cells) and walks them in that order, `on` workgroups of consecutive tiles per XCD turn (1 = the
 * default, 64), so that what runs on an XCD at a time -- one L2 -- sees one region of the map instead of one pose's whole scan.
 * Results do not depend on it.  Exported by librmclhip.so. */
rmclhip_status rmclhip_rcc_set_batch_order(rmclhip_rcc* rcc, int on);
/* TEST read-back of the order of the LAST batch launch this operator enqueued (find_batch, correct_batch, simulate with several poses;
 * tests/test_gpu_pose_batch.py): *n_out = its number of order entries, nposes x *ngroups_out (nullable; the workgroups of one pose) --
 * 0 when that launch went pose-major (world order off, fewer than two poses, more than 65 535 workgroups per pose).  keys_out[pose *
 * ngroups + g] = the sort key (cell 0 .. 4095) of workgroup g of that pose; order_out[s] = pose << 16 | g of the s-th workgroup of the
 * sorted list.  Host buffers of `cap` words each, filled after a stream synchronisation; either may be null, both null only queries n;
 * cap < n: RMCLHIP_ERR_INVALID.  The values live in the operator's scratch until its next batch launch.  Changes nothing; works
 * without the experiments library. */
rmclhip_status rmclhip_debug_batch_order(rmclhip_rcc* rcc, uint32_t* keys_out, uint32_t* order_out, size_t cap, uint32_t* n_out,
                                         uint32_t* ngroups_out);

/* TEST knob of the loopback communicator (rmclhip_comm_create_loopback): its all-reduce adds the ranks' contributions starting at
 * `first_rank` instead of rank 0 -- the freedom a real collective library has.  Whatever must not depend on the library's order of
 * summation is tested under several rotations (tests/test_gpu_distributed.py).  Exported by librmclhip.so. */
rmclhip_status rmclhip_comm_loopback_set_reduce_rotation(rmclhip_comm* comm, uint32_t first_rank);

/* debug trace of the sharded entry points (rmclhip_pf_update_sharded, _allgather_weights, _sharded_resample*): on = 1 starts (and
 * clears) the recording, on = 0 stops it; buf (nullable) receives what was recorded before this call.  Tokens: "E<r>" rank r's part of
 * a phase was enqueued, "W<r>" the host waited for rank r, "<phase>:" labels.  A phase that lets the devices run concurrently reads
 * "E0 E1 ... W0 W1 ..."; tests/test_gpu_distributed.py asserts that.  Works without the experiments library. */
rmclhip_status rmclhip_debug_trace(int on, char* buf, size_t cap);
/* how often, in this process, a host poller found ITS sequence number in a completion tag while the result words it read did not yet add
 * up to the tag's checksum -- the event the {sequence, xor} tag guards against (tools/tag_retries.py, profiles/r05_tag_handoff.txt) */
rmclhip_status rmclhip_debug_tag_retries(unsigned long long* retries_out);
/* MEASUREMENT aid of rmclhip_particles_init_uniform / _init_pose / _pack_visualization (tools/particle_init_time.py): on != 0 brackets
 * what those calls enqueue on this context -- the kernel, and the pack's copy to the host -- with two HIP events; last_ms (nullable)
 * receives the bracket of the last such call made while it was on (0 before any).  Off by default: two event records per call.
 * Works without the experiments library. */
rmclhip_status rmclhip_debug_particles_timing(rmclhip_ctx* ctx, int on, float* last_ms);
/* MEASUREMENT aid of rmclhip_pf_stein_step (tools/stein_time.py): on != 0 puts four HIP events at the borders of the LAST iteration's
 * three phases -- the drive | the cell list (clears, insert, decision, scan, scatter) | the pair sums and the move; last_ms3 (nullable,
 * three floats) receives the phases of the last call made while it was on (0 before any).  Off by default.  Works without the
 * experiments library. */
rmclhip_status rmclhip_debug_stein_timing(rmclhip_pf* pf, int on, float* last_ms3);
/* TEST aid of the handles' lifecycles (tests/test_gpu_lifecycle.py): the bytes of device memory and of pinned or host-mapped memory the
 * library's handles hold in this process right now, over every device (memory handed out by rmclhip_malloc is the caller's and is not
 * counted).  Two relaxed atomic counters kept where the library allocates and frees, which no per-call path does.  Destroying every
 * handle a piece of code made brings both back to what they were before it.  Exported by librmclhip.so; null: RMCLHIP_ERR_INVALID. */
rmclhip_status rmclhip_debug_live_bytes(uint64_t* device_bytes, uint64_t* host_bytes);

/* TEST hook of the rotation solve (tests/test_gpu_umeyama.py): out_host[i] = the solve of stats_host[i] by solver 0 = umeyama() on the
 * host (what rmclhip_umeyama_transform calls; ctx may be null), 1 = umeyama() on the device, 2 = umeyama_fast() on the device (the
 * moment-form loops' solve with refined reciprocals instead of divisions).  The device solvers run one thread per element, 64 threads
 * per block.  Any other solver: RMCLHIP_ERR_INVALID.  Works without the experiments library. */
rmclhip_status rmclhip_debug_solve(rmclhip_ctx* ctx, const rmclhip_cross_statistics* stats_host, uint32_t n, int solver,
                                   rmclhip_transform* out_host);

/* A/B of the robust scale selection (tools/robust_micp_time.py; ROBUST MICP of rmclhip.h): on != 0, every histogram pass recomputes
 * the residual from the correspondences; 0 (default), the first pass writes the keys to scratch and the others read those.  The selected
 * median is the same either way.  Process-wide.  Works without the experiments library. */
rmclhip_status rmclhip_debug_robust_select_recompute(int on);

#ifdef __cplusplus
}
#endif
#endif
