/*
 * icp_mi355x.h — C ABI of the MI355X-native (gfx950, HIP) frame-to-model ICP odometry hot path.
 *
 * Drop-in boundary for pyLiDAR-SLAM's `ICPFrameToModel` and the inner plugin seams it is built from.
 * Every entry point cites the reference interface it replaces (paths relative to the reference repo root).
 * Plain pointers and sizes only: no torch / numpy types cross this boundary.  All matrices are row-major 4x4 float.
 *
 * Pointers tagged `mem` may live on the host (ICP_MEM_HOST: the library stages them through HBM) or on the device
 * (ICP_MEM_DEVICE: e.g. `tensor.data_ptr()` of a torch-ROCm tensor; zero-copy).  All work is enqueued on the context's
 * stream (`icp_set_stream`, default stream otherwise); entry points that return values to the host synchronise that
 * stream before returning, the others are asynchronous.
 *
 * Threading: one context per odometry instance, calls on one context must be serialised by the caller (this is the
 * reference's contract too: a single-threaded frame loop, slam/odometry/odometry_runner.py:170-182).
 *
 * Return value: ICP_OK (0) or a negative icp_status; `icp_last_error(ctx)` gives the message.
 */
#ifndef ICP_MI355X_H
#define ICP_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icp_ctx icp_ctx;

typedef enum {
    ICP_OK = 0,
    ICP_ERR_INVALID_ARGUMENT = -1, /* maps to the reference's AssertionError (slam/common/utils.py:30-38) */
    ICP_ERR_HIP = -2,              /* HIP runtime failure (message in icp_last_error) */
    ICP_ERR_INVALID_JACOBIAN = -3, /* RuntimeError("Invalid Jacobian in Gauss Newton minimization"),
                                      slam/common/optimization.py:334-336 (|det H| < 1e-7) */
    ICP_ERR_EMPTY_MAP = -4,        /* nearest-neighbour search against an empty local map */
    ICP_ERR_NO_DEVICE = -5,        /* no gfx950 device visible: the product path never falls back to the CPU */
    ICP_ERR_EXCHANGE = -6          /* multi-GPU exchange: a peer did not deliver its normal equations in time */
} icp_status;

typedef enum { ICP_MEM_HOST = 0, ICP_MEM_DEVICE = 1 } icp_mem;

/* Robust weighting schemes of slam/common/optimization.py:210-226 (`_LS_SCHEME`). */
typedef enum {
    ICP_SCHEME_LEAST_SQUARE = 0, /* "default" / "least_square" :66-72 */
    ICP_SCHEME_HUBER = 1,        /* :76-97  */
    ICP_SCHEME_EXP = 2,          /* :101-117 */
    ICP_SCHEME_NEIGHBORHOOD = 3, /* :121-145 */
    ICP_SCHEME_GEMAN_MCCLURE = 4,        /* :149-166 */
    ICP_SCHEME_SQUARE_GEMAN_MCCLURE = 5, /* :170-187 */
    ICP_SCHEME_CAUCHY = 6                /* :191-208 */
} icp_scheme;

/* Target-point masking of `ICPFrameToModel.sample_points` (slam/odometry/icp_odometry.py:301-308):
 * rows containing a NaN are always skipped (remove_nan, :357); ICP_TARGETS_SKIP_NULL additionally skips zero-norm rows
 * (the "non-null pixels of the vertex map" case, :303-305).  Skipped rows contribute nothing, exactly as if removed. */
typedef enum { ICP_TARGETS_ALL = 0, ICP_TARGETS_SKIP_NULL = 1 } icp_target_mode;

/* Cost minimised by every alignment of the registration loop: RIGID_ALIGNMENT `mode` of the reference
 * (slam/odometry/alignment.py:200-208, selected at slam/odometry/icp_odometry.py:98). */
typedef enum {
    ICP_COST_POINT_TO_PLANE = 0, /* point_to_plane_gauss_newton: GaussNewtonPointToPlaneAlignment :80-127 */
    ICP_COST_POINT_TO_POINT = 1  /* point_to_point_gauss_newton: GaussNewtonPointToPointAlignment :143-189, one step
                                    of PointToPointCost linearised at x0 = 0 per ICP iteration; no map normals */
} icp_cost;

typedef struct {
    /* SphericalProjector(height, width, 3, up_fov, down_fov), slam/common/projection.py:426-445 */
    int32_t height;
    int32_t width;
    float up_fov;   /* degrees */
    float down_fov; /* degrees */
    /* ICPFrameToModelConfig, slam/odometry/icp_odometry.py:29-64 */
    int32_t max_num_alignments;
    float threshold_delta_pose;
    /* GaussNewtonPointToPlaneConfig.gauss_newton_config {scheme, sigma}, slam/odometry/alignment.py:69-77 */
    int32_t scheme; /* icp_scheme */
    float sigma;
    /* KdTreeLocalMapConfig, slam/odometry/local_map.py:243-251 */
    int32_t local_map_size;
    int32_t num_neighbors_normals;
    /* MI355X-side knobs (no reference counterpart) */
    float cell_size;   /* voxel-hash cell edge in metres; <= 0: auto-tuned towards ~10 map points per occupied cell.
                          Search results never depend on it (the search is exact), only speed does */
    int32_t max_rings; /* fine-level rings searched before the coarse level / exhaustive fallback (default 2; exactness is kept either way) */
    int32_t device;    /* HIP device ordinal */
    int32_t poll_every; /* host polls the device-side `done` flag every N iterations (0: never; implied by threshold <= 0) */
} icp_config;

typedef struct {
    float pose[16];     /* relative pose new frame -> map frame, `new_pose_matrix` of register_new_frame :299 */
    float params[6];    /* [tx,ty,tz,ex,ey,ez], `new_pose_params` :299 */
    int32_t iterations; /* number of align() calls made (= len(losses) :289) */
    int32_t converged;  /* 1 if stopped by ||dx|| < threshold_delta_pose (:292) or the residual-norm guard */
    int32_t status;     /* icp_status of the Gauss-Newton loop */
    int32_t num_targets; /* target rows that took part (after NaN / null masking) */
    int64_t normals_computed; /* map normals estimated during this registration (lazy cache, local_map.py:397-422) */
} icp_register_result;

/* ---- lifecycle ------------------------------------------------------------------------------------------------- */
void icp_default_config(icp_config* cfg);
/* ICPFrameToModel.__init__ (slam/odometry/icp_odometry.py:77-121) */
int icp_create(const icp_config* cfg, icp_ctx** out);
void icp_destroy(icp_ctx* ctx);
const char* icp_last_error(const icp_ctx* ctx);
const char* icp_version(void);
/* hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream */
int icp_set_stream(icp_ctx* ctx, void* hip_stream);
int icp_synchronize(icp_ctx* ctx);
/* MI355X-side tuning options by name (no reference counterpart; none of them changes a result, only the schedule — with ONE
 * exception, "carry_normals", which changes results by float32 rounding and says so):
 *   "nn_cache" 0 | 1 | 2 (2)        exact nearest-neighbour cache across ICP iterations (2: a missed entry seeds the search)
 *   "hit_records" 0 | 1 (0)         the first cache hit behind a search leaves a record — the winner's point, its normal and a
 *                                   bound on every OTHER map point — from which later iterations decide the hit with 48 coalesced
 *                                   bytes and no gather (the entry's candidate set only where the record does not certify);
 *                                   measured slower than the speculative gathers it replaces: off by default
 *   "late_from" n (-1: never)       fused launches from ICP iteration n on run the LATE kernel: the same iteration built for
 *                                   launches the hit records settle (64 registers, 33 KB of LDS: four workgroups per CU instead
 *                                   of two; the few queries left are searched by a wave each); needs "hit_records"; same bits;
 *                                   off by default: a frame whose queries still miss in those launches pays 20x
 *   "late_waves" 8 | 6 (8)          ... its build: 64 registers (four workgroups per CU) or 80 (three)
 *   "fuse_iteration" 0 | 1 (1)      search + rows + partial sums in one kernel when every normal is ready
 *   "iterate_dense" 0 | 1 (1)       64-register build of that kernel (the whole scan resident in one round of workgroups)
 *   "wave_misses" n (48)            workgroups with up to n cache misses search each of them with a whole wave
 *   "wave_misses_dense" n (4)       the same threshold in the 128-queries-per-block launches of the early iterations
 *   "narrow_from" n (0; -1: never)  from ICP iteration n on the fused kernel takes 512 queries per block, one lane each,
 *                                   instead of 128 with a 4-lane group each; same bits (round 3: 3 — the one-lane ball
 *                                   search of round 4 suits the 512-query shape from the first iteration on)
 *   "frame_seed" 0 | 1 (1)          the neighbours of the last frame seed the first iteration of the next one
 *   "exchange_timeout_ms" (5000)    how long a rank waits for its peers inside the in-library exchange
 *   "knn_rings" n (-1: auto), "knn_lanes" 2 | 4 (4), "target_occupancy" points per cell (16), "search_stats" 0 | 1 | 2 | 3 | 4 (0; dev: 3 / 4 = 1 / 2 + a per-workgroup dump on stderr)
 *   "cell_lists" 0 | 1 (0)          grid build: the table slots a build claims are listed; the next build empties those slots, not the
 *                                   whole table, and the cells' starts are scanned over the lists instead of over every slot
 *                                   (measured: slower for one map per launch, faster for a batch of maps — DESIGN §0)
 *   "scan_poll_limit" n (2^20)      grid build (without "cell_lists"): polls of a predecessor tile's descriptor before a tile of the one-launch table
 *                                   scan computes its prefix from the table itself (a safeguard; tests set 0 to walk that path)
 *   "prune_guard" m (0.002)         searches scan neighbour cells whose box is within m metres of the best distance instead of
 *                                   pruning them (the gap of a pruned cell bounds the cache's L: a guard keeps L off the best).
 *                                   Speed only: exactness does not rest on it.  Every box gap is taken short by 16 * 2^-24 *
 *                                   (|coordinate| + (|cell offset| + 1) * cell edge), which covers the few ulp by which cell
 *                                   membership (floorf(p / h)) and cell boxes (c * h) disagree; 0 gives the same bits
 *                                   (tests/test_gpu_search_audit.py; before that audit 0 could return a neighbour micrometres
 *                                   farther than the nearest, and the coarse level and knn_query, which have no guard, did)
 *   "refresh_at" n (2), "refresh_margin" m (2e-3)   in launch n, NN-cache entries with less slack than m are searched again
 *   "xcd_sectors" 0 | 1 (1)         the workgroups one XCD receives take one azimuth sector of the range image
 *   "lead_after_dense" 0 | 1 (1)    the first 512-query launch also solves the last 128-query one
 *   "lead_solve" 0 | 1 (1)          launched / unpolled registrations: the 6x6 solve of iteration k runs in an extra workgroup
 *                                   at the head of the (late, 512-queries-per-block) launch k + 1, which publishes the pose to
 *                                   the workgroups of that launch through a mailbox, instead of a launch of its own; same bits
 *   "resident_tail" n (0: never)    from ICP iteration n on (and never before the "wide_until" launches are through) ONE launch
 *                                   runs every remaining iteration of a launched / unpolled registration AND the solve behind the
 *                                   last one: its workgroups (one per CU, 512 queries each) stay resident, keep their queries'
 *                                   targets, cache entries and candidate sets in registers, take every pose from the mailbox and
 *                                   hand their partial rows to the lead — workgroup 0, which also takes its share of the queries
 *                                   — as tagged 8-byte granules; no launch boundary, no cold L2, no k_sum_solve launch per late
 *                                   iteration, and a loop with a live stop threshold ends on the device (no chunks).  Needs every
 *                                   workgroup resident at once (scans of up to 512 x CU count points); every wait is bounded by
 *                                   "lead_timeout_ms": on a GPU shared with foreign work a wait may run out — the registration is
 *                                   then finished on per-iteration launches (same bits) and the context keeps to those
 *                                   (icp_handoff_fallbacks counts such registrations); same bits.  OFF by default: measured at the
 *                                   headline size it costs 7 % (0.382 vs 0.357 ms per frame: what the launch boundary costs per
 *                                   late iteration, 1.1 us, is less than the tagged rows and the skew of 256 resident workgroups
 *                                   add), and nothing is gained on the published configuration's 12-workgroup scans
 *   "resident_tail_max_blocks" n (4096) ... for scans of up to n x 512 points
 *   "lead_timeout_ms" t (50)        wall-clock bound of that poll: a workgroup that does not see the pose in time gives up and
 *                                   the registration ends with ICP_ERR_HIP instead of hanging the GPU (the hand-off assumes the
 *                                   lead workgroup — blockIdx 0 — is dispatched before the pollers fill the machine; raise the
 *                                   bound, or set "lead_solve" 0, where a context shares its GPU with heavy foreign work)
 *   "ball_search" 0 | 1 (1)         NN-cache misses of the fused kernel are first searched by ONE lane each: own cell, then the
 *                                   cells across its nearer faces that a ball of the best distance reaches (99 % of the queries
 *                                   of an ordinary frame); whatever does not fit goes to the 4-lane / whole-wave searches; same
 *                                   bits.  With it the 512-query shape may serve the first iteration as well ("narrow_from" 0)
 *   "ball_lanes" 1 | 2 | 4 | 8 (8)  ... by 2 neighbouring lanes each where the workgroup has at most 256 misses, by 4 where it has
 *                                   at most 128, by 8 where it has at most 64 (the groups of four points of a cell alternate between the lanes, one butterfly
 *                                   merge of their sorted keys at the end); 1: one lane always, and workgroups with up to
 *                                   "wave_misses" misses go straight to the whole-wave search
 *   "ball_empty" 0 | 1 (1)          a miss whose own cell is EMPTY (no neighbour row to read) stays with the ball search when it
 *                                   brings a seed: the other seven cells of its 2x2x2 block by hashed probes, then the same
 *                                   pruning and scan (frames whose initial guess is half a metre off put a sixth of the scan
 *                                   into empty cells; 0: those queries go to the cooperative searches, round 5's schedule)
 *   "far_lanes" 0 | 16 (16)         what the ball search hands back (own cell empty, a ball that leaves its block, more than
 *                                   "ball_max" candidates) where a workgroup has more than "far_min" of them and at most
 *                                   "far_max": every such query searched by 16 lanes, THREADS / 16 queries at a time — seven
 *                                   cell lookups per lane in flight together, the points of the cells found 64 per round;
 *                                   0: the whole-wave / 4-lane searches take them; same bits
 *   "far_max" n (128)               see "far_lanes"
 *   "far_min" n (16)                see "far_lanes": more than n handed-back queries (up to n: a whole wave each)
 *   "wide_until" n (3)              the launches of ICP iterations below n run 1024 threads per 512 queries (two lanes for every
 *                                   miss even when all 512 search: the slowest wave of a launch is a lane walking the candidates
 *                                   of a dense cell alone); same bits
 *   "first_build" 0 | 1 (1)         icp_register_launch / icp_register_launch_from_last / icp_frame_launch of ONE sequence: ICP
 *                                   iteration 0 runs a build of the fused kernel of its own, which reads the scan rows itself,
 *                                   packs them for the later launches and initialises the registration state — no packing
 *                                   launch in front of it, no miss list in front of its searches (every query of that launch
 *                                   searches).  Taken with fused iterations, normals at hand (eager or carried), "ball_search",
 *                                   the 512-query shapes ("narrow_from" 0; "wide_until" > 0 with "ball_lanes" >= 2), and without
 *                                   the in-library exchange, "hit_records", "lazy_fused", "search_stats" and the event profile;
 *                                   otherwise, and with 0, the packing launch and the generic kernel run
 *                                   (icp_first_build_launches counts the registrations that took it); same bits
 *   "ball_max" n (256; <= 256)      ... if own cell + surviving cells hold at most n candidates: one lane walks them alone, and the
 *                                   longest walk of a launch sets its duration (heavier queries: the cooperative searches)
 *   "chunked_launch" 0 | 1 (1)      icp_register_launch with threshold_delta_pose > 0 enqueues as many iterations as the last
 *                                   registration ran, plus one; icp_register_end enqueues more while the loop is still running
 *   "flat_rows" 0 | 1 | 2 (2)       how the 4-lane search reads the neighbour cells that survive the box test: 2 = cell by cell,
 *                                   the four lanes striding each cell together; 1 = laid end to end and dealt out candidate by
 *                                   candidate; 0 = every lane walks its own cells (round 2's schedule)
 *   "hoods" 0 | 1 | 2 (2)           neighbourhood lists: the points of every occupied cell's 27-neighbourhood copied into one
 *                                   contiguous run at each grid build (<= 27 x 16 B per map point, maps up to 2^22 points whose
 *                                   normals will be estimated all at once, point-to-plane cost, 5 or 10 neighbours); the
 *                                   kNN normals stream ring 1 from it — 2: one lane per map point, sorted 32-bit keys, the
 *                                   uncertified points finished by a launch of their own, one wave each; 1: four lanes per point
 *                                   (round 3); 0: no lists, the 27 cells of the neighbour row are walked
 *   "carry_normals" 0 | 1 (1)       a POSE-ONLY map update (icp_map_update without a cloud and without an eviction: every map
 *                                   point keeps its neighbours) rotates the normals the grid already holds with the points
 *                                   (n' = R^-1 n) instead of clearing them; the reference clears its cache on every build_model
 *                                   (local_map.py:365-369) and re-estimates on first touch — the same vectors up to the float32
 *                                   rounding of the re-expressed points (poses agree to ~1e-7 m).  0: the reference's schedule,
 *                                   every rebuild clears the cache.  Updates that insert or evict always clear it
 *   "lazy_fused" 0 | 1 | 2 (0)      normals ON DEMAND inside the fused iteration kernel (KdTreeLocalMap.__get_normals' own schedule,
 *                                   local_map.py:397-422: estimate on first touch, cache until the next build_model): a query whose
 *                                   neighbour has no normal yet waits in its workgroup, whole waves estimate those normals behind
 *                                   the searches — the same exact kNN, covariance and eigen-solve as the all-at-once kernels: the
 *                                   same bits — and store them for every later launch.  1: where the map holds more than
 *                                   "lazy_fused_ratio" times the valid targets of the last registration (a grid-sampled frame
 *                                   against a window of key frames: 6 000 normals estimated instead of 180 000 per frame); 2:
 *                                   wherever the kernel exists (point-to-plane, 10 or 5 neighbours, one GPU); 0 (default): never
 *                                   — measured on the published configuration it moves 137 us of estimation from behind the map
 *                                   update (in the shadow of the host's next frame) onto the path to the pose: 0.55 vs 0.46 ms
 *   "lazy_fused_ratio" r (4)        see "lazy_fused"
 *   "overlap_map_update" 0 | 1 (0)  a map update that needs none of the context's scratch buffers — a pose-only update, or the
 *                                   insertion of a cloud staged with icp_map_stage_cloud — runs on a stream of the context's own,
 *                                   behind everything enqueued so far and beside what the caller enqueues next as long as that
 *                                   touches neither the map nor a registration: the upload, grid sample and projection of the
 *                                   next frame overlap the re-expression, grid rebuild and normal estimation of this one; every
 *                                   other entry point first orders the caller's stream behind the update.  Off by default:
 *                                   measured, the two event hand-offs between the streams cost more than the overlap returns
 *                                   (headline loop 2549 vs 2840 scans/s; published-configuration loop unchanged)
 *   "insert_by_cell" 0 | 1 (1)      behind a map update the points claim their cells of the new grid in the cell order of the
 *                                   previous grid (a rigid step leaves the points of an old cell in one or two new ones: the lanes
 *                                   of a wave share their claims) instead of in insertion order
 *   "clear_ahead" 0 | 1 (1)         a second hash table (+ 32 B per table slot: 4 MB at the headline sizes, 32 MB for a million
 *                                   map points, allocated at the first launched registration): extra workgroups of the last
 *                                   solving launch of an enqueued registration empty it beside the one workgroup that solves;
 *                                   the next grid build of that size inserts into it without a clearing pass and the tables
 *                                   change places.  A build that finds no clean spare of its size (no registration in front
 *                                   of it, a table that grew) clears in its own first launch as before; same bits
 *   "move_on_insert" 0 | 1 (1)      a build into a clean table has no clearing launch: the re-expression of the kept points, the
 *                                   carried normals, the NN cache -> seed conversion and two counter resets ride in the
 *                                   insertion launch (insert, scan, scatter: three launches per pose-only update); same bits
 *   "normals_list" 0 | 1 (0)        the stragglers of the eager kNN normals — the ~0.3 % of the map points whose k-th neighbour
 *                                   the pair pass does not certify — go to a list and a launch of their own right behind the
 *                                   estimating one: sixteen lanes per point, exact keys, DPP merges, ring 2 by hashed probes
 *                                   (0: each is finished by a whole wave of the workgroup that met it).  Same normals, bit for
 *                                   bit.  Off by default: measured, the pair pass alone takes 37 us and the stragglers' launch
 *                                   55 behind it, against 62 us with the stragglers inside (their chains overlap the other
 *                                   workgroups' pair passes there)
 *   "normals_tail_stream" 0 | 1 (0) the eager kNN normals behind a map update finish their stragglers (the ~0.2 % of the map
 *                                   points whose k-th neighbour ring 1 does not certify: a ~30 us chain of dependent probes
 *                                   each) on that stream of the context's own instead of inside the estimating launch: they run
 *                                   beside the next frame's preprocessing, and the next entry point that touches the map or a
 *                                   registration orders the caller's stream behind them.  Same normals, bit for bit.  Off by
 *                                   default: measured, neither the published-configuration loop (0.354-0.382 vs 0.360-0.366 ms
 *                                   per frame) nor the headline loop under the reference's schedule (2365-2374 vs 2370 scans/s)
 *                                   moves — behind a map update the GPU waits for the host's next upload, not the reverse
 *   "eager_normals_limit" m (2^20)  maps of up to m points get all their normals in one launch behind every map update (and
 *                                   the fused iteration kernel) whatever the scan size; larger maps only when m <= 2 n
 *   "profile_rotate" 0 | 1 (0)      icp_profile_enable brackets one iteration launch per registration (see icp_profile_read_iterations)
 *   "profile_every" n (1)           icp_profile_enable times the kernels of every n-th registration only (an event pair
 *                                   costs ~2 us of stream time: 40 pairs per frame are 10 % of a 0.8 ms registration)
 * The library reads no environment variables. */
int icp_set_option(icp_ctx* ctx, const char* name, double value);
/* runtime re-configuration of the alignment (RIGID_ALIGNMENT.load, slam/odometry/alignment.py:200-208).  Like icp_set_option and
 * icp_set_cost: iterations a chunked launch holds back are enqueued first, and the call is refused ("registration in
 * progress") between icp_register_begin and icp_register_end (a longer loop would re-allocate the state the iterations run on) */
int icp_set_alignment(icp_ctx* ctx, int32_t scheme, float sigma, int32_t max_num_alignments,
                      float threshold_delta_pose);
/* the alignment mode of the registration loop (icp_cost; default point to plane) */
int icp_set_cost(icp_ctx* ctx, int32_t cost);

/* ---- projection: Projector.build_projection_map (slam/common/projection.py:331-418) ------------------------------
 * xyz [n,3] -> vertex map [3,H,W] planar (zeros where empty), nearest point wins each pixel.
 * index_out (optional, [H*W] int32): winning point index per pixel, -1 where empty. */
int icp_project(icp_ctx* ctx, const float* xyz, int64_t n, int mem, float* vmap_out, int32_t* index_out, int out_mem);
/* The same projection for the DEVICE-RESIDENT pipeline (device pointers only): vmap_out [3,H,W] as above and rows_out
 * [H*W,3] = the same pixels as rows, i.e. vmap.permute(1, 2, 0).reshape(-1, 3) — what ICPFrameToModel.sample_points
 * (slam/odometry/icp_odometry.py:301-308) indexes and the registration takes as targets — written by the same launch
 * instead of a transposing copy per frame. */
int icp_project_rows(icp_ctx* ctx, const float* xyz, int64_t n, float* vmap_out, float* rows_out);
/* torch__spherical_projection (slam/common/projection.py:11-73): float pixel coordinates rows/cols [n] (diagnostics) */
int icp_project_pixels(icp_ctx* ctx, const float* xyz, int64_t n, int mem, float* rows_out, float* cols_out,
                       int out_mem);

/* ---- dataset side: KITTIOdometrySequence.correct_scan (slam/dataset/kitti_dataset.py:202-231) ----------------------
 * scan [n, stride] float32 rows (stride = 4 for KITTI's x, y, z, reflectance .bin records, 3 for plain xyz) ->
 * corrected xyz [n,3] float64 (the reference's einsum promotes to float64). */
int icp_kitti_correct_scan(icp_ctx* ctx, const float* scan, int64_t n, int stride, int mem, double* xyz_out, int out_mem);

/* ---- voxel grid sampling: voxelise / voxel_hashing / sample_from_hashes (slam/common/pointcloud.py:13-79,170-195),
 * GridSample.filter (slam/preprocessing.py:213-226) -----------------------------------------------------------------
 * indices_out [>= n] int64: original index of the first point of every distinct voxel hash, ordered by ascending
 * int64 hash; *count_out = number of samples; points_out (optional) [count,3] gathered samples. */
int icp_grid_sample(icp_ctx* ctx, const float* xyz, int64_t n, int mem, double voxel_size, int64_t* indices_out,
                    float* points_out, int64_t* count_out, int out_mem);
/* voxel coordinates [n,3] int64 and hashes [n] int64 (either output may be NULL) */
int icp_voxel_hash(icp_ctx* ctx, const float* xyz, int64_t n, int mem, double voxel_size, int64_t* voxels_out,
                   int64_t* hashes_out, int out_mem);

/* float64-input variants: `GridSample` applied to the float64 output of `Distortion` (config/slam/preprocessing/
 * grid_sample.yaml: distortion -> grid_sample on "distorted"); points_out is float64 [count,3] */
int icp_grid_sample_f64(icp_ctx* ctx, const double* xyz, int64_t n, int mem, double voxel_size, int64_t* indices_out,
                        double* points_out, int64_t* count_out, int out_mem);

/* The same selections for the DEVICE-RESIDENT pipeline (device pointers only; no reference counterpart beyond GridSample
 * itself): nothing is read back to the host — no synchronisation, every launch asynchronous on the context's stream.  The
 * outputs hold n rows: the V samples first (ascending int64 hash, as above), then NaN points and index -1; V goes to
 * *count_out, a DEVICE int32 (NULL: not reported).  Consumers that mask NaN rows — icp_project, the registration entry
 * points, icp_map_stage_cloud / icp_map_update — take the padded array as it is: a frame then needs ONE synchronisation, the
 * one that hands its pose to the host. */
int icp_grid_sample_padded(icp_ctx* ctx, const float* xyz, int64_t n, double voxel_size, int64_t* indices_out,
                           float* points_out, int32_t* count_out);
int icp_grid_sample_padded_f64(icp_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int64_t* indices_out,
                               double* points_out, int32_t* count_out);

/* Voxelization.filter / voxel_normal_distribution (slam/preprocessing.py:63-98, slam/common/pointcloud.py:83-167):
 * voxel coordinates [n,3] and hashes [n] (optional), voxel_ids_out [n] = rank of the point's hash among the distinct
 * hashes, *num_voxels_out = V, and (all three or none) sizes_out [V] int64 point counts, means_out [V,3] float32,
 * covs_out [V,3,3] float32 = sum (p - mean)(p - mean)^T (unnormalised, as in the reference), voxels ordered by
 * ascending int64 hash.  Per-voxel outputs must hold n entries (V <= n). */
int icp_voxel_statistics(icp_ctx* ctx, const float* xyz, int64_t n, int mem, double voxel_size, int64_t* voxels_out,
                         int64_t* hashes_out, int64_t* voxel_ids_out, int64_t* num_voxels_out, int64_t* sizes_out,
                         float* means_out, float* covs_out, int out_mem);

/* ---- de-skew: Distortion.filter (slam/preprocessing.py:144-191) --------------------------------------------------
 * Every point moves by the fraction alpha = (t - t_min) / (t_max - t_min) of the initial motion estimate `rel_pose`:
 * out = slerp(I, R, alpha) p + alpha t  (alpha = 0 when all timestamps are equal).  xyz [n,3] float32, timestamps [n]
 * float64, rel_pose row-major 4x4 float64, out [n,3] float64 (the reference's einsum promotes to float64).
 * R is the rotation scipy's Rotation.from_matrix yields for the 3x3 block handed over, as the reference's Slerp takes it: a
 * block that is not a rotation to 1e-12 — a pose that went through float32, as the constant-velocity guess of the frame
 * calls does — is replaced by its orthogonal factor first, then read as a quaternion (Markley).  RANGE  held to the reference
 * (scipy's Slerp and a float64 einsum) within 7.6e-15 of |p| + |t| per point — 4 x that reference's own float64-against-
 * long-double difference, 9e-13 m at 120 m — for theta from 0 to pi - 1e-6, exact float64 and float32-rounded poses alike
 * (tests/test_gpu_preprocess_audit.py; theta = 1e-4 / 0.05 / 0.3 / 1 / 3 rad, 4000 points at 40 m, float32 pose: 4e-14 ..
 * 1e-13 m from the reference).  theta -> pi is OUTSIDE it: at pi the quaternion's w is 0 up to rounding and its sign, which
 * the reference's own SVD and this library's iteration round differently, decides the way round of the interpolation.
 * (The log map of the raw matrix this entry point used before, (R - R^T) / 2 and the trace, was 1.6e-11 / 5.4e-8 / 4.9e-7 /
 * 1.4e-6 / 1.8e-5 m off the reference at those five angles for a float32 pose, and for an exact float64 pose 1.6e-11 m at
 * pi - 1e-3, 1.4e-8 m at pi - 1e-6 and 80 m at pi, where its axis vanished.)  A NaN timestamp is not defined here: numpy's
 * min / max hand it on to every point, the device's fmin / fmax drop it. */
int icp_distort(icp_ctx* ctx, const float* xyz, const double* timestamps, int64_t n, int mem, const double rel_pose[16],
                double* xyz_out, int out_mem);

/* ---- time stamps of a rotating sensor: estimate_timestamps (slam/common/geometry.py:443-466) ------------------------
 * rows [n, stride] float32 (stride = 3 for xyz rows, 4 for the x, y, z, reflectance records of a .bin scan) ->
 * timestamps [n] float64 in [0, 1]: the producer of the `timestamps` pointer icp_distort, the four frame calls and
 * icp_batch_preprocess take (in device memory: no host round trip).  ARITHMETIC  The reference, on float32 rows, stays in
 * float32:  phi = arctan2(y, x) * (clockwise ? -1 : +1);  phi -= float32(phi_0);  phi += float32(2 pi) where phi < 0;
 * t = (phi - min phi) / (max phi - min phi).  numpy's float32 arctan2 is not correctly rounded (one ulp, 2.4e-7, off the
 * rounded float64 value in about a third of the rows; time stamps 1.8e-7 apart), so no kernel matches it bit for bit.  The
 * library evaluates atan2 in float64, rounds ONCE to float32 — the correctly rounded value — and then follows the
 * reference in float32, operation by operation; the float32 quotient is widened to float64 (min maps to exactly 0, max to
 * exactly 1, so the renormalisation inside the de-skew is the identity on it).  RANGE  within 4 x the reference's own
 * float32-rows-against-float64-rows difference of every row (tests/test_timestamps_audit.py measures it,
 * tests/test_gpu_timestamps.py holds the kernels to it and, bit for bit, to a numpy model of the arithmetic above).
 * SEAM  y = +0 / -0 with x < 0 gives +pi / -pi: with phi_0 = pi, clockwise, both end at exactly 0.  A row within about
 * 1.5e-7 rad of the seam but not on it gets 0 or 1 depending on the last bit of arctan2 — the reference's own float32 and
 * float64 evaluations disagree there — and is outside the range above.  One row, or rows that all share one azimuth:
 * 0 / 0 = NaN for every row, as in the reference.  A NaN coordinate is not defined here: numpy's min / max hand it on to
 * every row, the device's fmin / fmax drop it (that row gets NaN, the others are unaffected).
 * Refused (ICP_ERR_INVALID_ARGUMENT, with a message): n <= 0 (the reference raises on an empty scan), a stride other than
 * 3 or 4, and a call while a registration or a frame of the context is in flight (shared scratch, as for the alignment
 * seams).  Two launches; with device input and output the stream is never waited on. */
int icp_estimate_timestamps(icp_ctx* ctx, const float* rows, int64_t n, int stride, int mem, int clockwise, double phi_0,
                            double* timestamps_out, int out_mem);
/* KITTI360Sequence.__getitem__ (slam/dataset/kitti_360_dataset.py:170-185): what the reference's KITTI-360 reader does to
 * one raw scan — KITTIOdometrySequence.correct_scan and estimate_timestamps (there: clockwise, phi_0 = pi) — from ONE
 * read of the scan, in the same two launches.  xyz_out [n,3] float64: the bits of icp_kitti_correct_scan; timestamps_out
 * [n] float64: the bits of icp_estimate_timestamps (arithmetic, seam, NaN cases and refusals as stated there). */
int icp_kitti360_prepare(icp_ctx* ctx, const float* scan, int64_t n, int stride, int mem, int clockwise, double phi_0,
                         double* xyz_out, double* timestamps_out, int out_mem);

/* ---- local map: KdTreeLocalMap (slam/odometry/local_map.py:254-427) ----------------------------------------------
 * Every call that changes the map (icp_map_init, icp_map_set, the icp_map_update family) first enqueues the iterations a
 * chunked launch holds back, and is refused ("registration in progress") between icp_register_begin and icp_register_end: the
 * caller's next icp_iteration_accumulate would search a grid that is gone or rebuilt. */
int icp_map_init(icp_ctx* ctx);                                             /* init()               :279-288 */
int icp_map_set(icp_ctx* ctx, const float* xyz, int64_t m, int mem);        /* set_map_pointcloud() :289-299 */
/* update() :302-362 — move the map by inv(rel), append `new_xyz` (rows with NaN dropped; NULL / n = 0: pose-only
 * update), evict the oldest cloud beyond local_map_size, rebuild the search structure and clear the normal cache.
 * *inserted_out (optional) = number of rows appended.  rel_pose = NULL: the pose of the last registration on this
 * context, read on the device (no host round trip; valid after icp_register / icp_register_launch).  If that
 * registration stopped on an error (ICP_ERR_INVALID_JACOBIAN, ICP_ERR_EXCHANGE) the map is NOT moved (the reference
 * raises before it would touch the map; the error itself reaches the caller through icp_register_end).  While the
 * result of a launched registration is still pending, only the pose-only form (new_xyz = NULL) is accepted with
 * rel_pose = NULL: an insertion / eviction must not follow a registration whose status the host has not seen. */
int icp_map_update(icp_ctx* ctx, const float rel_pose[16], const float* new_xyz, int64_t n, int mem, int row_mode,
                   int64_t* inserted_out);
/* The same update in two steps, for a caller that knows BEFORE a registration which cloud it will insert after it
 * (ICPFrameToModel.do_process_next_frame inserts the frame it has just registered, icp_odometry.py:229-231,360-376):
 * icp_map_stage_cloud flags and compacts the valid rows (row_mode as above) into the context and sends their count to the
 * host without waiting for it; icp_map_update_staged then performs update() :302-362 with those rows — same map, same
 * *inserted_out — and has nothing to wait for when anything that synchronises (icp_register_end) ran in between: one host
 * round trip per frame less than icp_map_update with a cloud.  A staged cloud is consumed by the first
 * icp_map_update_staged and replaced by the next icp_map_stage_cloud; rel_pose = NULL as for icp_map_update.  Both are refused
 * ("a frame is launched and awaits its end") between icp_frame_launch and icp_frame_end (or the projective pair): the staged rows
 * are then the frame's, which a key frame's end inserts. */
int icp_map_stage_cloud(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int row_mode);
int icp_map_update_staged(icp_ctx* ctx, const float rel_pose[16], int64_t* inserted_out);
/* update(new_vertex_map=...) :320-324 — appends the pixels of a [3,H,W] vertex map with norm > 0.01 */
int icp_map_update_vertex_map(icp_ctx* ctx, const float rel_pose[16], const float* vmap, int mem,
                              int64_t* inserted_out);
int64_t icp_map_size(const icp_ctx* ctx);
int icp_map_num_clouds(const icp_ctx* ctx);
/* registrations of this context that were finished on per-iteration launches because a hand-off between workgroups ran out
 * of its wall-clock budget ("resident_tail", "lead_solve": a GPU shared with foreign work); the first one switches the
 * context to per-iteration launches for good — results are unaffected (diagnostics; no reference counterpart) */
int icp_handoff_fallbacks(const icp_ctx* ctx);
/* registrations of this context whose first launch was the first-iteration build (option "first_build") instead of the packing
 * launch + the generic kernel (diagnostics; no reference counterpart) */
int icp_first_build_launches(const icp_ctx* ctx);
/* registrations of this context whose launches were latched onto lead launches when they began (icp_register_begin and what
 * builds on it, icp_batch_register_launch): no other context of the process was registering on the device at that moment.  One
 * finished by the recovery behind a timed-out hand-off stays counted (diagnostics; no reference counterpart) */
int icp_lead_registrations(const icp_ctx* ctx);
/* contexts of this process that are in a registration against the kd-tree style map, or hold an uncollected result of one, on
 * `device` right now: what the decision above looks at.  -1 outside 0..63 (diagnostics; no reference counterpart) */
int icp_registering_contexts(int device);
int icp_map_get(icp_ctx* ctx, float* xyz_out, int out_mem); /* current map [M,3] in insertion order */
/* nearest_neighbor_search() :372-395 + __get_normals :397-422 — exact Euclidean 1-NN (no distance cap) and the
 * lazily estimated normal of every hit.  Outputs [n,3], [n,3], [n] (any may be NULL). */
int icp_nearest_neighbor_search(icp_ctx* ctx, const float* xyz, int64_t n, int mem, float* neighbor_points_out,
                                float* neighbor_normals_out, int32_t* neighbor_index_out, int out_mem);
/* KDTree(map).query(xyz, k) — pykdtree.kdtree.KDTree as the reference builds and queries it (slam/odometry/local_map.py:369,
 * 385, 405) — against the kd-tree style map of the context (icp_map_set / icp_map_update*): the exact k nearest map points
 * of n ARBITRARY query rows xyz [n,3], no distance cap.
 *   order      ascending by (d2, original map index): exact distance ties go to the lower index.  d2 is float32,
 *              fma(dz,dz, fma(dy,dy, dx*dx)) of the float32 coordinate differences.
 *   outputs    dist_out [n,k] float32: sqrtf(d2), or d2 itself under ICP_KNN_SQR_DISTS; index_out [n,k] int32: indices into
 *              the map in the insertion order icp_map_get returns.  Either may be NULL, not both.
 *   missing    when fewer than k neighbours exist (the map holds fewer than k points, or the bound below leaves fewer) the
 *              remaining entries are dist = +inf, index = icp_map_size() — scipy's and pykdtree's convention.  A query row
 *              with a NaN or infinite coordinate has no neighbours: k missing entries.
 *   bound      distance_upper_bound = b > 0 keeps only neighbours with d2 < b*b (float32 product), strictly: a point exactly
 *              at the bound is excluded, as scipy.spatial.cKDTree does.  b <= 0 or +inf: no bound.
 *   k          1..32.  The search options ("cell_size", max_rings, "knn_rings") never change a result.
 * ICP_ERR_EMPTY_MAP on an empty map; ICP_ERR_INVALID_ARGUMENT (icp_last_error says why) for k outside 1..32, n < 0, both
 * outputs NULL, unknown flags, or a registration or frame that is in flight or uncollected.  Iterations a chunked launch
 * still holds back are enqueued first.  The call reads the grid only: normals, the nearest-neighbour cache, the
 * registration state and the staged buffers of a frame are left as they were (it stages through buffers of its own).
 * n = 0 returns ICP_OK and writes nothing.  Not available: a batched form, radius / ball queries, k > 32. */
#define ICP_KNN_SQR_DISTS 1
int icp_knn_query(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int32_t k,
                  float distance_upper_bound /* <= 0 or +inf: none */, int32_t flags,
                  float* dist_out, int32_t* index_out /* either may be NULL */, int out_mem);
/* Test support for the search schedule (no reference counterpart; the reference recomputes every neighbour in every
 * iteration, slam/odometry/icp_odometry.py:274-297): the ORIGINAL map index of the point each target of the last
 * registration was matched with in its LAST iteration (-1: masked row), read back from the exact nearest-neighbour cache
 * the fused iteration kernel keeps, and rows 0-2 of the pose that iteration ran with (pose_out, host memory, may be
 * NULL).  Valid right after icp_register / icp_register_end, before the map changes; ICP_ERR_INVALID_ARGUMENT otherwise. */
int icp_last_neighbors(icp_ctx* ctx, int32_t* neighbor_index_out, float pose_out[12], int out_mem);
/* Test support for the certificates of that cache (no reference counterpart): the entry of every target of the last
 * registration as its last fused launch left it.  An entry is a candidate set S of up to three map points and a lower
 * bound L on the distance from the target, at the pose of the iteration that searched it, to every map point NOT in S; a
 * later iteration keeps it while sqrt(d2_winner) * 1.000001 < L - (|displacement| * 1.000001 + 1e-7) - margin.
 *   members_out           [n,3] int32: ORIGINAL map indices, the stored neighbour first, -1: none
 *   bound_out             [n] float32: L (0: the entry certifies nothing)
 *   search_iteration_out  [n] int32: the iteration of the search, the 7-bit field resolved to the largest j <= last with
 *                         j = field (mod 128); -1 for masked rows and empty entries (members -1, L 0)
 *   records_out           [n,8] float32, only under option "hit_records" (ICP_ERR_INVALID_ARGUMENT otherwise): the two
 *                         float4 of the row's hit record, (winner xyz, bound), (normal, bits(iteration of the bound; -1: none));
 *                         a device pointer must be 16-byte aligned
 *   pose_hist_out         HOST memory, [last + 1, 12] float32: rows 0-2 of the pose of every iteration 0 .. last
 *   last_iteration_out    HOST memory: `last`, the iteration icp_last_neighbors reports (call with the other outputs NULL
 *                         to size pose_hist_out)
 * Every output may be NULL.  Valid and refused in the states of icp_last_neighbors (icp_last_error says which); reads the
 * targets, the entries, the map points and the records, and stages through a buffer of its own: the cache, the normals and
 * the registration state are left as they were. */
int icp_last_cache_entries(icp_ctx* ctx, int32_t* members_out, float* bound_out, int32_t* search_iteration_out,
                           float* records_out, float* pose_hist_out, int32_t* last_iteration_out, int out_mem);

/* ---- projective local map: ProjectiveLocalMap (slam/odometry/local_map.py:91-240), the reference's "GPU" variant -----
 * compute_normal_map (slam/common/geometry.py:240-295): vertex map [3,H,W] -> normal map [3,H,W] (box-filter plane fit,
 * zero where the pixel is null or |det| <= 1e-6). */
int icp_compute_normal_map(icp_ctx* ctx, const float* vmap, int mem, int kernel_size, float* nmap_out, int out_mem);
/* compute_neighbors (slam/common/geometry.py:397-439): per pixel the closest of k_maps reference vertex maps
 * [k_maps,3,H,W] to the target map [3,H,W] (null pixels never match; ties -> the first map); optionally gathers
 * ref_fields [k_maps,c_fields,H,W] along.  neighbors_out [3,H,W], fields_out [c_fields,H,W]. */
int icp_compute_neighbors(icp_ctx* ctx, const float* tgt_vmap, const float* ref_vmaps, const float* ref_fields,
                          int k_maps, int c_fields, int mem, float* neighbors_out, float* fields_out, int out_mem);
/* icp_pmap_init and icp_pmap_update are refused ("a frame is launched and awaits its end") between the two frame calls of the
 * context: the window is the one the frame registers against and its end re-expresses and appends to. */
int icp_pmap_init(icp_ctx* ctx); /* init() :113-119 */
/* update() :122-174 — re-express the kept maps by inv(rel_pose), append `vmap` [3,H,W] with its normal map (NULL:
 * pose-only update), drop the oldest beyond local_map_size, rebuild the model (build_model :177-202). */
int icp_pmap_update(icp_ctx* ctx, const float rel_pose[16], const float* vmap, int mem, int normals_kernel_size);
int icp_pmap_num_maps(const icp_ctx* ctx);
/* the model: `_model_vmap` / `_model_nmap` as [K, H*W, 4] float rows (xyz + valid flag, normal + 0) */
int icp_pmap_get_model(icp_ctx* ctx, float* model_v4_out, float* model_n4_out, int out_mem);
/* nearest_neighbor_search() :205-235 — projective association of the (already transformed) points xyz [n,3]:
 * rows9_out [count,9] = neighbour point, neighbour normal, target point per matched pixel, in pixel order. */
int icp_pmap_nearest_neighbor_search(icp_ctx* ctx, const float* xyz, int64_t n, int mem, float* rows9_out,
                                     int64_t* count_out, int out_mem);
/* register_new_frame (slam/odometry/icp_odometry.py:248-299) against the projective map; same contract as
 * icp_register.  Refused (ICP_ERR_INVALID_ARGUMENT) while a registration of the context is in progress or a launched one
 * awaits icp_register_end: the call collects through the result slots, oldest first, and would hand out that older result. */
int icp_pmap_register(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16],
                      icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out);

/* ---- rigid alignment: GaussNewtonPointToPlaneAlignment.align (slam/odometry/alignment.py:91-127) on given
 * correspondences; one Gauss-Newton step from x0 = 0 (slam/common/optimization.py:296-344).
 * dx_out[6], pose_out[16] = build_pose_matrix(dx), loss_out = sum (w r)^2, normal_eq_out (optional) = 32 doubles:
 * 21 upper-triangular JtJ, 6 Jtr, sum (w r)^2, sum r^2, row count, 2 pad; residuals_out (optional, [n] float, in the
 * memory space `mem` of the inputs) = (w r)^2 per row, the residual tensor `align` returns (optimization.py:342-344).
 * The outputs are written before ICP_ERR_INVALID_JACOBIAN is returned (dx = 0, the loss and the sums of the rows).
 * Refused with ICP_ERR_INVALID_ARGUMENT ("registration in progress") between icp_register_begin / icp_register_launch and
 * icp_register_end: the call stages into the target, partial-row and normal-equation buffers of the registration. */
int icp_align_point_to_plane(icp_ctx* ctx, const float* ref_points, const float* tgt_points, const float* ref_normals,
                             int64_t n, int mem, float dx_out[6], float pose_out[16], double* loss_out,
                             double* normal_eq_out, float* residuals_out);

/* GaussNewtonPointToPointAlignment.align (slam/odometry/alignment.py:143-189) on given correspondences: one
 * Gauss-Newton step of PointToPointCost (slam/common/optimization.py:458-560) linearised at x0 (NULL = zeros; with
 * `initialize_with_svd` the caller passes from_pose_matrix(icp_weighted_procrustes(...))).  params_out = x0 + dx,
 * pose_out = build_pose_matrix(params_out); loss_out / normal_eq_out / residuals_out as above.  Refused with "registration
 * in progress" like icp_align_point_to_plane. */
int icp_align_point_to_point(icp_ctx* ctx, const float* ref_points, const float* tgt_points, int64_t n, int mem,
                             const float x0[6], float params_out[6], float pose_out[16], double* loss_out,
                             double* normal_eq_out, float* residuals_out);
/* weighted_procrustes (slam/common/registration.py:15-74): closed-form rigid transform target -> reference.  weights
 * [n] float32 or NULL (ones); as in the reference they enter the centroids only.  pose_out row-major 4x4 float64.
 * Refused with "registration in progress" like icp_align_point_to_plane. */
int icp_weighted_procrustes(icp_ctx* ctx, const float* tgt_points, const float* ref_points, const float* weights,
                            int64_t n, int mem, double pose_out[16]);

/* ---- registration: ICPFrameToModel.register_new_frame (slam/odometry/icp_odometry.py:248-299) --------------------
 * All iterations run on the device without host round trips.  loss_per_iter_out / dx_per_iter_out (optional) receive
 * `iterations` entries ([.] double, [.,6] float). */
int icp_register(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16],
                 icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out);

/* Device-side helper of ICPFrameToModel.sample_points for vertex-map targets (slam/odometry/icp_odometry.py:301-308:
 * `target_points[target_points.norm(dim=-1) > 0.0]`) without a host round trip for the count: the rows of xyz [n,3]
 * that pass `target_mode` (rows with a NaN never do; null rows do not under ICP_TARGETS_SKIP_NULL) are written, in
 * order, to the head of out [cap,3]; the rest of `out` is zero-filled, so registering `out` with ICP_TARGETS_SKIP_NULL
 * registers exactly the passing rows — with cap instead of n rows to walk (a 64x2048 vertex map built from a 6000-point
 * grid sample has at most 6000 non-null pixels).  Both pointers are device memory.  cap must be >= the number of passing
 * rows (the caller knows such a bound by construction); passing rows beyond cap are dropped.  Asynchronous. */
int icp_compact_targets(icp_ctx* ctx, const float* xyz, int64_t n, int target_mode, float* out, int64_t cap);

/* ---- multi-GPU seam: one ICP iteration split around the exchange of the packed normal equations -------------------
 * begin -> { accumulate -> [all-reduce the 32 doubles at icp_normal_equations_ptr over RCCL] -> solve } x iters -> end.
 * Every rank registers its own slice of the target points against a replicated map and applies the identical solve.*/
int icp_register_begin(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16]);
/* begin + every iteration enqueued + the result copied to pinned host memory behind the last iteration, without waiting:
 * work enqueued afterwards on the same context (icp_map_update with rel_pose = NULL: the pose-only branch of
 * ICPFrameToModel.__update_map, icp_odometry.py:379) overlaps the host's wait in icp_register_end, which then blocks on
 * the registration only.  With threshold_delta_pose > 0 only a first chunk of iterations is on the stream when this
 * returns ("chunked_launch": as many as the last registration ran, plus one; launches behind an early stop are
 * device-side no-ops); icp_register_end enqueues more while the loop is still running.
 * CALLS BEFORE icp_register_end.  Every entry point of this header belongs to one class while a launched registration is
 * enqueued or uncollected (tests/inflight_audit.py holds the class of each, state by state, and tests/test_gpu_inflight_audit.py
 * holds the library to it):
 *   ORDERED (enqueues them first): icp_map_update, icp_map_update_staged, icp_map_stage_cloud, icp_map_set, icp_map_init,
 *       icp_map_update_vertex_map, icp_set_option, icp_set_cost, icp_set_alignment, icp_set_stream,
 *       icp_set_normal_equations_buffer, icp_map_normals_owned / _install, icp_odometry_init, icp_register_launch,
 *       icp_register_launch_from_last.
 *     Each changes what the held-back iterations would see, so it first enqueues ALL of them: the stream order is the call
 *     order, as if every iteration had been enqueued here, and the call takes effect behind the registration.  (A third
 *     launch is refused: two results may be pending.)  The batched forms do the same for every member.
 *   REFUSED (while a registration is enqueued or uncollected): icp_register, icp_register_begin, icp_pmap_register,
 *       icp_pmap_register_launch, icp_nearest_neighbor_search, icp_knn_query, icp_last_neighbors, icp_last_cache_entries,
 *       icp_align_point_to_plane, icp_align_point_to_point, icp_weighted_procrustes, icp_estimate_timestamps,
 *       icp_kitti360_prepare, icp_map_normals_peek, icp_exchange_create / _connect / _destroy, icp_iteration_accumulate,
 *       icp_iteration_solve, icp_frame_launch, icp_frame_end, icp_pmap_odometry_init, icp_pmap_frame_launch, icp_pmap_frame_end.
 *     ICP_ERR_INVALID_ARGUMENT, icp_last_error names the reason, nothing changed.  They share the targets, the partial rows, the
 *     normal equations, the state or the staging scratch with the registration, or need its result slot (icp_knn_query
 *     enqueues the held-back iterations before it refuses).
 *   INDEPENDENT: everything else that launches work — the projection, the grid samples, icp_voxel_hash / _statistics,
 *     icp_distort, icp_kitti_correct_scan, icp_compact_targets, icp_compute_normal_map, icp_compute_neighbors, the projective
 *     map (icp_pmap_init, icp_pmap_update, icp_pmap_get_model, icp_pmap_nearest_neighbor_search), icp_map_get, icp_synchronize,
 *     the profile, aggregated maps, elevation images, refiners.  They stage through buffers no iteration reads (an iteration
 *     reads the packed targets, the grid, the normals, the NN cache, the state, the partial rows and the mailbox) and run in
 *     stream order behind what is enqueued; held-back iterations stay held back.
 *   COLLECTS: icp_register_end (the oldest result first).
 * Between icp_register_begin and icp_register_end only icp_iteration_accumulate / _solve, icp_set_stream,
 * icp_set_normal_equations_buffer and the INDEPENDENT calls are accepted (the padded grid samples are refused there too). */
int icp_register_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16]);
/* the same with the initial guess = the pose of the previous registration on this context, READ ON THE DEVICE: the
 * constant-velocity initialisation (`ConstantVelocityInitialization`, slam/initialization.py:103-119 — the last relative
 * pose) without the host in the loop.  Up to two launched registrations may await their icp_register_end (which returns
 * them oldest first), so a frame loop can enqueue frame t + 1 (and the map update by the device-resident pose of frame
 * t) before it has collected the pose of frame t: the GPU never idles between frames while the host still receives
 * every pose, one frame later. */
int icp_register_launch_from_last(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode);
/* search + normals + reduce into the 32-double device vector: 21 upper-triangular JtJ, 6 Jtr, sum (w r)^2, sum r^2, the
 * count of valid rows, and two pad elements (30, 31) that are always 0.0.  A rank whose slice is empty (n = 0) or holds
 * only masked rows (NaN; (0,0,0) under ICP_TARGETS_SKIP_NULL) writes EXACT ZEROS into elements 0 .. 29 — never what an
 * earlier iteration or registration left there — so any cut of a scan may be registered, a world larger than the scan
 * included, and the Invalid-Jacobian test applies to the summed system alone (a slice that is singular on its own is no
 * error).  Elements 27 and 28 are sums of float64 products of the float32 operands on the fused path and of float32
 * squares on the unfused and the point-to-point path (1e-8 apart).  Behind the end of the loop (the stop threshold, a
 * guard or an error decided by icp_iteration_solve, identically on every rank) both calls return without writing: a
 * driver may go on calling accumulate / all-reduce / solve for a fixed iteration count — the vector then holds stale
 * sums that grow world-fold per all-reduce, which nothing reads: the result is that of the stopping iteration, and
 * icp_register_begin starts the next registration from a vector that every accumulate overwrites
 * (tests/test_gpu_sharded_audit.py). */
int icp_iteration_accumulate(icp_ctx* ctx);
int icp_iteration_solve(icp_ctx* ctx);      /* 6x6 solve + pose update from the (possibly all-reduced) vector */
/* collects the registration in progress, or the OLDEST launched one.  Refused with a message: nothing to collect; a batch that
 * still holds iterations of this context back (icp_batch_register_end collects it); a frame launched on the context, by itself
 * or by a batch ("a frame is launched and awaits its end": icp_frame_end / icp_pmap_frame_end / the batch's end collect it). */
int icp_register_end(icp_ctx* ctx, icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out);
void* icp_normal_equations_ptr(icp_ctx* ctx); /* device pointer, 32 doubles */
/* use caller-owned device memory (e.g. a torch tensor RCCL can reduce in place) for the 32-double vector; iterations a chunked
 * launch holds back are enqueued first (they sum into the vector they were launched with) */
int icp_set_normal_equations_buffer(icp_ctx* ctx, void* device_ptr);

/* ---- one call per odometry frame: ICPFrameToModel.do_process_next_frame (slam/odometry/icp_odometry.py:157-246) ------
 * The frame loop of the reference behind two calls, for the kd-tree style map and either cost: what a caller otherwise
 * composes from ten entry points above — the upload, the de-skew (Distortion.filter, slam/preprocessing.py:144-191), the
 * grid sample (GridSample.filter :207-226) and its float32 cast (ToTensor :101-126), the projection and the choice of the
 * targets (_read_input / sample_points, icp_odometry.py:319-358), the registration from the constant-velocity guess
 * (ConstantVelocityInitialization, slam/initialization.py:103-119), the key-frame test and the map update (__update_map,
 * icp_odometry.py:360-380) and the copy-out of `odometry_pc`.  The calls compose the entry points above in the order
 * pylidar_slam_amd/odometry.py::MI355XICPFrameToModel issues them: per frame the same pose, parameters, iteration count,
 * losses, steps, insertions and map, bit for bit.  No kernel of its own.
 *   icp_odometry_init  ICPFrameToModel.init (:128-145): icp_map_init, frame counter 0, the motion since the last key frame
 *                      and the last relative pose = identity.  Calling it again starts a new sequence on the same context
 *                      (a frame launched and not ended is collected and dropped).
 *   icp_frame_launch   enqueues one frame on the context's stream and returns without waiting.
 *                      INPUT  xyz [n,3] float32.  ICP_MEM_HOST: one host copy into a pinned buffer of the context, one DMA
 *                      on an upload stream of the context's own into one of two alternating device slots, the context's stream
 *                      made to wait for it; a slot is overwritten by the frame after next — its last reader is the
 *                      registration of its own frame, collected by then (icp_frame_end); `xyz` (and `timestamps`) are free
 *                      when the call returns.  ICP_MEM_DEVICE: the rows are used in place and must stay untouched until
 *                      icp_frame_end has returned.  timestamps [n] float64 live where xyz lives.
 *                      DE-SKEW  with `timestamps` and an initial guess — init_pose, or the last relative pose under
 *                      constant_velocity (identity for frames 0 and 1) — the frame is de-skewed by that guess (icp_distort)
 *                      into float64 rows; without a guess (constant_velocity = 0 and init_pose = NULL) the frame passes through,
 *                      as Distortion does without `init_rpose` (:157-162).
 *                      GRID SAMPLE  voxel_size > 0: icp_grid_sample_padded of the float32 rows, or icp_grid_sample_padded_f64 of
 *                      the de-skewed float64 rows followed by the (float)x cast — the chain icp_batch_preprocess documents, for
 *                      one member.  Nothing is read back: the frame keeps its n rows, the samples first, NaN rows behind them.
 *                      FRAME 0  projection and icp_map_update_vertex_map(identity, vertex map) (:176); no registration.
 *                      LATER FRAMES  targets = 1: icp_project_rows, the targets are the pixels of the vertex map with
 *                      ICP_TARGETS_SKIP_NULL (sample_points :301-308); targets = 0: the targets are the frame's rows and the
 *                      vertex map — which the kd-tree branch reads nowhere behind frame 0 — is NOT built (the plugin builds it
 *                      behind the registration and drops it).  Then icp_map_stage_cloud of the frame's rows (stage_max_rows), the
 *                      copy of the staged rows towards the host on a stream of its own (copy_cloud), and icp_register_launch_from_last —
 *                      under constant_velocity with init_pose = NULL, from frame 2 on, while the device still holds the last
 *                      frame's pose — or icp_register_launch (init_pose; the last relative pose; identity).
 *   icp_frame_end      icp_register_end: an error status (ICP_ERR_INVALID_JACOBIAN) is returned before the map is touched, as
 *                      the reference raises at :286 — the frame counter, the last pose and the motion since the last key frame
 *                      stay as they were.  Then __update_map (:360-380) on the host: new_delta = delta x pose in float32, its
 *                      Euler parameters (Pose.from_pose_matrix, slam/common/pose.py:120-207), key frame when |t| >
 *                      threshold_trans or |r| 180 / pi > threshold_rot; icp_map_update_staged (icp_map_update with the rows for a
 *                      frame that was not staged) for a key frame (delta = identity),
 *                      the pose-only icp_map_update otherwise (delta = new_delta) — enqueued, not waited for.
 *                      odometry_pc_out (optional, `cap` rows, out_mem) receives the frame's valid rows in order (rows with a
 *                      NaN dropped, :357: for a grid-sampled frame its samples), *rows_out their count (0 for a frame that was
 *                      neither staged nor asked for its cloud: nobody counted its rows); more rows than `cap`:
 *                      ICP_ERR_INVALID_ARGUMENT with the count in *rows_out and nothing written — the frame is completed all the
 *                      same (result filled, map updated).  Frame 0 writes no rows, as the reference writes none (:171-181).
 *                      loss_per_iter_out / dx_per_iter_out as for icp_register_end.
 * ICP_ERR_INVALID_ARGUMENT with a message, the context usable as before: a context that holds a projective map, an exchange or
 * profiling switched on, a context held by a batch, icp_frame_launch before icp_odometry_init or while a frame awaits its
 * icp_frame_end, icp_frame_end with nothing launched.
 * CALLS BETWEEN icp_frame_launch AND icp_frame_end (and between icp_pmap_frame_launch and icp_pmap_frame_end) follow the
 * classes of icp_register_launch, with the frame's own registration, staged rows and window taken out of the caller's reach:
 * icp_register_end, icp_map_stage_cloud, icp_map_update_staged, icp_pmap_init and icp_pmap_update are REFUSED there ("a frame
 * is launched and awaits its end": they would collect the frame's result, replace or consume the rows a key frame inserts,
 * or move the window its end appends to), icp_frame_end / icp_pmap_frame_end COLLECT, and icp_odometry_init /
 * icp_pmap_odometry_init collect and drop the frame.  The ORDERED calls stay ORDERED — an explicit icp_map_update,
 * icp_set_option, icp_set_alignment take effect behind the frame's registration and in front of the update its end enqueues.
 * One frame at a time per context; B contexts step together through icp_batch_frame_launch /
 * icp_batch_frame_end below. */
typedef struct icp_frame_config {
    double voxel_size;         /* > 0: GridSample (slam/preprocessing.py:207-226) in front of the frame; <= 0: the rows as given */
    float threshold_trans;     /* key-frame test, metres (ICPFrameToModelConfig.threshold_trans, icp_odometry.py:29-64: 0.1) */
    float threshold_rot;       /* key-frame test, degrees (threshold_rot: 0.3) */
    int32_t constant_velocity; /* 1: initial guess = the last relative pose (slam/initialization.py:103-119); 0: identity */
    int32_t targets;           /* 0: the frame's rows; 1: the pixels of its vertex map (sample_points, icp_odometry.py:301-308) */
    int32_t copy_cloud;        /* 1: icp_frame_end will be asked for odometry_pc in host memory: its copy starts in
                                  icp_frame_launch, beside the registration; 0: copied (if asked for) inside icp_frame_end */
    int32_t stage_max_rows;    /* frames of more rows are NOT staged in front of their registration (a 131 072-row frame pays
                                  more for the compaction on the way to its pose than the round trip behind it costs): a key
                                  frame then goes in through icp_map_update with the rows.  Same map either way.  <= 0: always
                                  staged; grid-sampled frames always are.  Default 32768 */
} icp_frame_config;
typedef struct icp_frame_result {
    icp_register_result reg; /* frame 0: identity pose, zero parameters, 0 iterations */
    int32_t frame_index;     /* 0 for the first frame behind icp_odometry_init */
    int32_t key_frame;       /* 1: the frame went into the map (frame 0 always does) */
    int64_t samples;         /* rows behind the grid sample (voxel_size <= 0: n) */
    int64_t inserted;        /* rows appended to the map (0 for a pose-only update) */
} icp_frame_result;
void icp_default_frame_config(icp_frame_config* cfg);
int icp_odometry_init(icp_ctx* ctx, const icp_frame_config* cfg);
int icp_frame_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, const double* timestamps,
                     const float init_pose[16]);
int icp_frame_end(icp_ctx* ctx, icp_frame_result* result, float* odometry_pc_out, int64_t cap, int64_t* rows_out,
                  int out_mem, double* loss_per_iter_out, float* dx_per_iter_out);

/* ---- B sequences per launch: batched registration ------------------------------------------------------------------
 * The reference registers ONE sequence, one frame at a time (ICPFrameToModel.register_new_frame,
 * slam/odometry/icp_odometry.py:248-299; one `SLAM` object per process, slam/slam.py:84-163): a chain of dependent,
 * latency-bound iterations that leaves most of an MI355X idle.  A batch ties B contexts of ONE device — B independent
 * sequences, each with its own local map, scan and registration state — together so that iteration k of all B
 * registrations is ONE kernel launch ("HBM-bound operation is only approachable by batching many
 * independent registrations per launch"): the per-sequence arguments sit in a descriptor table in device memory, every
 * sequence has a lead workgroup of its own, and one host thread enqueues the launches of all B.  Per sequence the
 * arithmetic is that of icp_register_launch on the same context with the same options: the same poses, bit for bit.
 *   icp_batch_create           ties `count` contexts (1..ICP_BATCH_MAX_SEQUENCES, same device, same alignment configuration
 *                              — max_num_alignments, scheme, sigma — and same schedule options) together; they stay usable on
 *                              their own between batched calls and must outlive the batch;
 *   icp_batch_set_stream       icp_set_stream on every member (a batch enqueues everything on ONE stream);
 *   icp_batch_register_launch  icp_register_launch (from_last = 0; init_poses = count x 16 floats or NULL: identity) or
 *                              icp_register_launch_from_last (from_last = 1) on every member: xyz[b] / n[b] = member b's
 *                              scan.  With a forced iteration count every iteration is enqueued; with a live stop
 *                              threshold a first chunk (as many as the slowest member ran last time, plus one), further
 *                              chunks from icp_batch_register_end while a member is still running — a member whose loop has
 *                              ended idles on the device.  While the batch holds iterations back its members refuse the
 *                              single-context entry points (ICP_ERR_INVALID_ARGUMENT).  Point-to-plane registrations on the
 *                              fused path only (eager normals, no exchange, no profiling): ICP_ERR_INVALID_ARGUMENT otherwise.
 *                              SHARED OPTIONS: one launch runs one kernel instantiation for all members and one host loop
 *                              decides how many iterations go onto the stream, so besides the stream, max_num_alignments,
 *                              scheme and sigma the members must have EQUAL values of threshold_delta_pose (equal, not only
 *                              both zero or both live: the chunks are sized for one stop test) and of the options
 *                              chunked_launch, lead_after_dense, hit_records, late_from, late_waves, wide_until, narrow_from,
 *                              nn_cache and ball_search.  A difference is refused before any member changes
 *                              (ICP_ERR_INVALID_ARGUMENT, icp_batch_last_error names the option; no scan imported, no map or
 *                              pose touched, nothing enqueued: every member registers on its own afterwards as if the call
 *                              had not been made).  Every other option is the member's own and travels in its descriptor: the
 *                              ball / far search options (ball_lanes, ball_empty, ball_max, far_lanes, far_min, far_max),
 *                              wave_misses, refresh_at, refresh_margin, frame_seed, xcd_sectors and everything that steers the
 *                              map update (carry_normals, normals_list, knn_lanes, cell_lists) may differ from member to
 *                              member; lead launches run when every member allows them (lead_solve).  A launch that fails
 *                              after the checks (a member that cannot take the fused path, a HIP error) gives the
 *                              registration up: no member stays in registration or held by the batch.
 *                              icp_batch_pmap_register_launch applies the same rule;
 *   icp_batch_project          icp_project for every member in two launches: xyz[b] [n[b],3] -> vmap_out[b] [3,H,W] of member b
 *                              (Projector.build_projection_map, slam/common/projection.py:331-418, as ICPFrameToModel._read_input
 *                              calls it per frame, icp_odometry.py:333); DEVICE pointers only;
 *   icp_batch_map_update       icp_map_update(member, NULL, NULL, ...) for every member: the pose-only update by the
 *                              device-resident pose of the registration just launched (icp_odometry.py:379) — the B grid
 *                              rebuilds in four launches (held-back iterations are enqueued first: the update reads the END of
 *                              the registration);
 *   icp_batch_map_update_staged  ICPFrameToModel.__update_map (slam/odometry/icp_odometry.py:360-380) for every member:
 *                              insert[b] != 0: KdTreeLocalMap.update (slam/odometry/local_map.py:302-362) with the cloud member
 *                              b staged by icp_map_stage_cloud — move the map by inv(rel), append the staged rows, evict the
 *                              oldest cloud beyond local_map_size, rebuild, clear the normal cache (then the eager normals, as
 *                              icp_map_update_staged); insert[b] == 0: the pose-only update (as icp_batch_map_update;
 *                              "carry_normals" applies).  rel_poses = count x 16 floats, or NULL: every member's device-resident
 *                              pose of its last registration.  inserted_out (optional, count entries): rows appended per
 *                              member (0 for a pose-only member).  Per member the same map, window, normals and later
 *                              registrations, bit for bit, as icp_map_update_staged(member, rel, ...) /
 *                              icp_map_update(member, rel, NULL, ...) on that member alone.  The B grid builds take four or
 *                              five launches, the neighbourhood lists ONE, the eager normals ONE per neighbourhood size (members
 *                              whose normals another kernel computes — "knn_lanes" 2, "hoods" < 2, "normals_list" 1,
 *                              "normals_tail_stream" 1, another num_neighbors_normals — get their own launch, as on their own).
 *                              Every member is checked before any changes: ICP_ERR_INVALID_ARGUMENT, nothing changed, when a
 *                              member is on another stream, an inserting member has no staged cloud, or rel_poses = NULL while a
 *                              member never registered or an inserting member's registration has not been collected
 *                              (icp_batch_register_end).  Held-back iterations are enqueued first;
 *   icp_batch_pmap_register_launch  icp_pmap_register (the reference's ProjectiveLocalMap.nearest_neighbor_search + the
 *                              Gauss-Newton step per ICP iteration, slam/odometry/local_map.py:205-235, icp_odometry.py:248-299)
 *                              against every member's projective map, enqueued, collected by icp_batch_register_end:
 *                              xyz[b] / n[b] = member b's targets, init_poses = count x 16 floats or NULL (identity), or
 *                              from_last = 1 (the device-resident pose of the member's previous registration).  All
 *                              max_num_alignments iterations are enqueued for all members — ONE launch in front (targets,
 *                              states, z-buffers), then three per iteration (projection of the targets, association + rows +
 *                              partial sums, sum + solve) — a member whose loop has ended does nothing on the device; no host
 *                              polls.  Per member the same result, losses and steps, bit for bit, as icp_pmap_register on that
 *                              member alone.  Every member is checked before any changes: ICP_ERR_EMPTY_MAP when a member has
 *                              no projective map; ICP_ERR_INVALID_ARGUMENT when members are on different streams, differ in
 *                              max_num_alignments, scheme, sigma, height, width or field of view, a member's registration is
 *                              still pending (icp_batch_register_end / icp_register_end first) or a member holds kd-tree
 *                              iterations back (chunked launches), or runs point-to-point, an exchange or profiling;
 *   icp_batch_pmap_update      icp_pmap_update (ProjectiveLocalMap.update, slam/odometry/local_map.py:122-202) for every member:
 *                              rel_poses = count x 16 floats (required); vmaps[b] ([3,H,W], `mem`) inserts member b's vertex
 *                              map with its normal map (normals_kernel_size), vmaps[b] = NULL (or vmaps = NULL) is a pose-only
 *                              update; the first update of an empty map needs a vertex map.  The window (poses re-expressed in
 *                              double precision, eviction beyond local_map_size) is kept on the host as icp_pmap_update keeps
 *                              it; on the device ONE launch inserts the new maps (normal map fused with the store), three
 *                              rebuild the models of every (member, slot) pair, whatever the window size.  Per member the same
 *                              window and model, bit for bit, as icp_pmap_update on that member alone.  Every member is checked
 *                              before any changes (ICP_ERR_INVALID_ARGUMENT, nothing changed): one stream, one image geometry,
 *                              no pending registration, no held-back kd-tree iterations, a vertex map for an empty map, a
 *                              regular relative pose;
 *   icp_batch_register_end     icp_register_end for every member (results[b]; loss_per_iter_out / dx_per_iter_out:
 *                              count x max_num_alignments (x 6) entries or NULL): ONE wait for all of them.  Returns the
 *                              first member's non-zero status, every member's own in results[b].status.
 * The stage in front of them — every call below follows the same rules: DEVICE pointers only, everything enqueued on the
 * batch's stream behind what each member already has there (iterations the batch or a member still holds back are enqueued
 * first), every member checked before anything is enqueued (ICP_ERR_INVALID_ARGUMENT, nothing enqueued, no member changed,
 * when a member is on another stream, is inside a registration — icp_register_begin .. icp_register_end — or its arguments
 * are inconsistent), nothing read back:
 *   icp_batch_preprocess       the reference's Preprocessing chain Distortion -> GridSample -> ToTensor(float32)
 *                              (slam/preprocessing.py:144-191, :207-226, :101-126; the chain :269-290) for frames[b] of every
 *                              member b, with the padded grid sample of icp_grid_sample_padded[_f64].  A frame with
 *                              `timestamps` ([n] float64) is de-skewed by rel_pose (as icp_distort) into distorted_out ([n,3]
 *                              float64, required exactly then) and sampled from those float64 rows; a frame without (NULL:
 *                              Distortion's pass-through) is sampled from its float32 rows.  samples_out (optional): the n
 *                              padded sample rows in the frame's element type (float64 when de-skewed, float32 otherwise) —
 *                              the V samples by ascending voxel hash, NaN rows behind them; samples_f32_out (required when
 *                              n > 0): the same rows cast to float32 ((float)x); indices_out (optional): [n] int64, -1 behind
 *                              the samples; count_out (required): V, an int32 on the device.  Per member the same bits as
 *                              icp_distort + icp_grid_sample_padded[_f64] + a float32 cast on that member alone.  Two launches
 *                              de-skew the members that have timestamps, four sample every member (one per kernel kind for the
 *                              whole batch); a frame of more than 262 144 points takes the single path in the same call;
 *   icp_batch_project_rows     icp_project_rows (Projector.build_projection_map, slam/common/projection.py:331-418, as
 *                              ICPFrameToModel._read_input calls it per frame, slam/odometry/icp_odometry.py:319-358) for every
 *                              member in two launches: xyz[b] [n[b],3] -> vmap_out[b] [3,H,W] and rows_out[b] [H*W,3] (rows_out
 *                              or rows_out[b] NULL: the vertex map only, as icp_batch_project);
 *   icp_batch_stage            icp_map_stage_cloud (the frame's valid rows, compacted and counted in front of its registration,
 *                              for the insertion of slam/odometry/icp_odometry.py:229-231) for every member in two launches:
 *                              xyz[b] [n[b],3] (NULL when n[b] == 0), row_mode ICP_TARGETS_*; every member's count lands in its
 *                              pinned word, its staged event is recorded: icp_batch_map_update_staged / icp_map_update_staged
 *                              consume the staged clouds as after icp_map_stage_cloud. */
#define ICP_BATCH_MAX_SEQUENCES 32
typedef struct icp_batch icp_batch;
int icp_batch_create(icp_ctx* const* ctxs, int32_t count, icp_batch** out);
void icp_batch_destroy(icp_batch* batch);
const char* icp_batch_last_error(const icp_batch* batch);
int icp_batch_set_stream(icp_batch* batch, void* hip_stream);
int icp_batch_register_launch(icp_batch* batch, const float* const* xyz, const int64_t* n, int mem, int target_mode,
                              const float* init_poses, int from_last);
int icp_batch_project(icp_batch* batch, const float* const* xyz, const int64_t* n, float* const* vmap_out);
int icp_batch_map_update(icp_batch* batch);
int icp_batch_map_update_staged(icp_batch* batch, const float* rel_poses, const int32_t* insert, int64_t* inserted_out);
int icp_batch_pmap_register_launch(icp_batch* batch, const float* const* xyz, const int64_t* n, int mem, int target_mode,
                                   const float* init_poses, int from_last);
int icp_batch_pmap_update(icp_batch* batch, const float* rel_poses, const float* const* vmaps, int mem,
                          int normals_kernel_size);
int icp_batch_register_end(icp_batch* batch, icp_register_result* results, double* loss_per_iter_out,
                           float* dx_per_iter_out);
typedef struct icp_preprocess_frame {
    const float* xyz;         /* [n,3] float32 */
    int64_t n;
    const double* timestamps; /* [n] float64, or NULL: no de-skew */
    double rel_pose[16];      /* the initial motion estimate (read when timestamps is set) */
    double* distorted_out;    /* [n,3] float64: required exactly when timestamps is set */
    void* samples_out;        /* optional: [n,3] padded samples, float64 when de-skewed, float32 otherwise */
    float* samples_f32_out;   /* [n,3] float32 copy of the padded samples (required when n > 0) */
    int64_t* indices_out;     /* optional: [n] int64 */
    int32_t* count_out;       /* required: V */
} icp_preprocess_frame;
int icp_batch_preprocess(icp_batch* batch, const icp_preprocess_frame* frames, double voxel_size);
/* estimate_timestamps (slam/common/geometry.py:443-466) for every member in two launches (device memory): per member the
 * bits of icp_estimate_timestamps — its arithmetic, seam band, all-equal-azimuth NaN and NaN-coordinate deviation hold
 * here.  A member with n[b] == 0 or a NULL scan sits out; refused: a stride other than 3 or 4, no member with rows, members
 * on different streams, a registration or a frame in flight on a member. */
int icp_batch_estimate_timestamps(icp_batch* batch, const float* const* rows, const int64_t* n, int stride, int clockwise,
                                  double phi_0, double* const* timestamps_out);
int icp_batch_project_rows(icp_batch* batch, const float* const* xyz, const int64_t* n, float* const* vmap_out,
                           float* const* rows_out);
int icp_batch_stage(icp_batch* batch, const float* const* xyz, const int64_t* n, int row_mode);

/* ---- one call per odometry frame, B sequences per call -----------------------------------------------------------------
 * icp_frame_launch / icp_frame_end for the members of a batch: the frame loop of B drives behind two calls, every launch
 * the batched one of the entry points above.  Per member the calls give what icp_frame_launch / icp_frame_end give on that
 * member's context alone with the same frames, bit for bit: pose, parameters, iteration count, losses, steps, key-frame
 * decision, samples, inserted, odometry_pc, map, window and every later frame.  No kernel of its own.
 *   icp_batch_odometry_init  icp_odometry_init(member, cfg) on every member, every member checked before any is restarted.  The sequence state — motion since the last
 *                      key frame, last relative pose, frame index, settings — is the MEMBER's: a member may be stepped by
 *                      the batch, then alone with icp_frame_launch / icp_frame_end, then by the batch again, and may be
 *                      restarted alone with icp_odometry_init(member, cfg) between two steps.
 *   icp_batch_frame_launch  frames[b] = member b's next frame (`mem`: where every xyz / timestamps lives).  skip != 0: the
 *                      member sits this step out — nothing of it is read, enqueued or changed.  The other members fall into
 *                      two groups.  FIRST FRAME (frame index 0): member by member what icp_frame_launch does for frame 0 (its
 *                      projection and icp_map_update_vertex_map); no registration.  REGISTERING (frame index >= 1), in
 *                      icp_frame_launch's order with ONE call per stage for the whole group: the uploads from host arrays,
 *                      icp_batch_preprocess for a group that grid-samples (members with timestamps and a guess are de-skewed
 *                      in the same call, the others pass through; icp_frame_launch's rule for the guess; without a grid sample
 *                      a de-skewed member takes icp_distort's launch and the float32 cast), icp_batch_project_rows
 *                      (targets = 1), icp_batch_stage, the copies of the staged rows and sample counts towards the host on a
 *                      stream of the batch's own, and icp_batch_register_launch — from_last = 1 when every registering member
 *                      would take icp_register_launch_from_last on its own, the host guesses otherwise (the same bits).
 *                      The batched form always stages: stage_max_rows is not consulted (the same map either way).
 *                      Host arrays travel through ONE pinned buffer, ONE upload stream and two alternating device buffers of
 *                      the batch, whatever the member count; odometry_pc through ONE pinned buffer and ONE copy stream.
 *   icp_batch_frame_end  icp_batch_register_end for the registering group, each member's key-frame test
 *                      (ICPFrameToModel.__update_map, slam/odometry/icp_odometry.py:360-380, as icp_frame_end applies it), then
 *                      icp_batch_map_update_staged over the members whose registration succeeded.  results[b] as
 *                      icp_frame_end fills it; a skipped member's is zeroed with frame_index = -1.  loss_per_iter_out /
 *                      dx_per_iter_out: count x max_num_alignments (x 6) entries as for icp_batch_register_end, or NULL.
 *                      odometry_pc_out (NULL, or count pointers of which any may be NULL), cap[b] rows each, rows_out[b]
 *                      (optional) as for icp_frame_end.
 * A FAILED REGISTRATION (ICP_ERR_INVALID_JACOBIAN) leaves its member as icp_frame_end leaves a single context: the map
 * untouched, the sequence not advanced, the device pose given up; every other member completes its frame.  The call returns
 * the first such status, every member's own is in results[b].reg.status.  cap[b] below the member's row count: the single
 * call's rule per member — ICP_ERR_INVALID_ARGUMENT, the count in rows_out[b], nothing written for that member, every frame
 * completed.
 * REFUSALS, checked for every member before any member changes (ICP_ERR_INVALID_ARGUMENT, icp_batch_last_error names the
 * member and the reason, nothing enqueued, every sequence where it was): a non-skipped member without a sequence; a launch
 * while a launch awaits its end; an end with nothing launched; every member skipped; a member that runs point-to-point (the
 * batch registers point-to-plane only), holds a projective map, an exchange or profiling, is in or awaits a registration or
 * a frame of its own; non-skipped members that differ in voxel_size or targets (one batched preprocessing and one target
 * mode per step); members on different streams.  A refusal's message ends in "(nothing was changed)"; every other status of
 * icp_batch_frame_end comes back behind a completed step.  A frame the batch has launched is ended by the batch: icp_frame_end and
 * icp_odometry_init on such a member are refused until then, and so are the single calls a member refuses between its own frame
 * calls (icp_register_end, icp_map_stage_cloud, icp_map_update_staged).
 * MEMBERS WITH WORK OF THEIR OWN: icp_batch_stage, icp_batch_map_update, icp_batch_map_update_staged, icp_batch_pmap_update,
 * icp_batch_pmap_register_launch and icp_batch_register_end are refused, before any member changes, while a member has launched
 * a frame of its OWN ("a frame is launched and awaits its end": the member's end collects that registration and inserts those
 * rows); icp_batch_register_launch, icp_batch_map_update and icp_batch_map_update_staged also while a member is between
 * icp_register_begin and icp_register_end ("registration in progress"). */
typedef struct icp_batch_frame {
    const float* xyz;          /* [n,3] float32, host or device (the call's `mem`) */
    int64_t n;
    const double* timestamps;  /* [n] float64 where xyz lives, or NULL */
    const float* init_pose;    /* 16 floats (host) or NULL: as icp_frame_launch */
    int32_t skip;              /* != 0: this member sits the step out; nothing of it is read, enqueued or changed */
} icp_batch_frame;
int icp_batch_odometry_init(icp_batch* batch, const icp_frame_config* cfg);
int icp_batch_frame_launch(icp_batch* batch, const icp_batch_frame* frames, int mem);
int icp_batch_frame_end(icp_batch* batch, icp_frame_result* results, float* const* odometry_pc_out, const int64_t* cap,
                        int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out);

/* ---- one call per odometry frame against the projective local map (PF2M) --------------------------------------------------
 * ICPFrameToModel.do_process_next_frame (slam/odometry/icp_odometry.py:157-246) with `ProjectiveLocalMap`
 * (slam/odometry/local_map.py:113-235) behind two calls, as icp_frame_launch / icp_frame_end give it for the kd-tree style map:
 * the calls compose the entry points above in the order pylidar_slam_amd/odometry.py::MI355XICPFrameToModel issues them for a
 * projective map — per frame the same pose, parameters, iteration count, losses, steps, key-frame decision, odometry_pc, window
 * and model, bit for bit.  Entry points, a config struct and a sequence state of their own: icp_odometry_init and
 * icp_frame_config know nothing of the projective map.
 *   icp_pmap_register_launch  icp_pmap_register (register_new_frame :248-299 against ProjectiveLocalMap.nearest_neighbor_search,
 *                      local_map.py:205-235), enqueued: begin + every iteration on the context's stream, the result copied to
 *                      pinned memory behind the last one and collected by icp_register_end.  The stop (threshold_delta_pose) is
 *                      decided on the device — the kernels of an iteration behind it return at once — and the host polls
 *                      nothing.  Pose, parameters, iterations, losses, steps and status are those of icp_pmap_register, bit for
 *                      bit.  One registration at a time (ICP_ERR_INVALID_ARGUMENT while one is in progress or awaits
 *                      icp_register_end).  Every iteration is on the stream when the call returns, so entry points called before
 *                      icp_register_end run in call order behind it, as icp_register_launch documents; those that need the
 *                      registration's outcome on the host (icp_pmap_update takes the pose) come after icp_register_end.
 *   icp_pmap_odometry_init  ICPFrameToModel.init (:128-145): icp_pmap_init, frame counter 0, the motion since the last key frame
 *                      and the last relative pose = identity.  Calling it again starts a new sequence on the same context (a
 *                      frame launched and not ended is collected and dropped).
 *   icp_pmap_frame_launch  enqueues one frame and returns without waiting.  `layout`:
 *                      ICP_FRAME_ROWS  data = [n,3] float32 rows in host or device memory (`mem`), timestamps [n] float64 where
 *                      the rows live: the chain of icp_frame_launch — upload through the pinned buffer and two device slots,
 *                      de-skew by the guess (icp_distort), grid sample (voxel_size > 0) and float32 cast — then the projection
 *                      (_read_input :319-358).  targets = 1: icp_project_rows, the targets are the pixels of the vertex map
 *                      with ICP_TARGETS_SKIP_NULL (sample_points :301-308); targets = 0: the targets are the frame's rows, and
 *                      the vertex map (which only a key frame's insertion reads) is projected BEHIND the registration.
 *                      ICP_FRAME_VERTEX_MAP  data = a [3,H,W] float32 vertex map in DEVICE memory, n = H*W (the reference's
 *                      default data_key, :319-344): the targets are its pixels with ICP_TARGETS_SKIP_NULL, transposed to rows
 *                      by one launch; timestamps or voxel_size > 0 are refused with this layout.  A device input must stay
 *                      untouched until icp_pmap_frame_end has returned.
 *                      FRAME 0  icp_pmap_update(identity, vertex map) (:176); no registration.
 *                      LATER FRAMES  the frame's valid rows are compacted and counted for odometry_pc (rows with a NaN dropped,
 *                      :357; vertex-map input: null pixels dropped as well, :342-344; input order kept), copied towards pinned
 *                      memory on a stream of the context's own (copy_cloud) beside the registration, and the registration is
 *                      enqueued (icp_pmap_register_launch) from init_pose, or the last relative pose under constant_velocity,
 *                      or the identity.
 *   icp_pmap_frame_end  icp_register_end: an error status (ICP_ERR_INVALID_JACOBIAN) is returned before the map or the sequence
 *                      state moves (:286).  Then __update_map (:360-380): the key-frame test of icp_frame_end, unchanged;
 *                      icp_pmap_update with the frame's vertex map for a key frame (local_map.py:122-174), pose-only
 *                      otherwise — enqueued, not waited for.  result->inserted = 1 when a vertex map was appended, else 0;
 *                      samples, odometry_pc_out, cap, *rows_out, loss_per_iter_out, dx_per_iter_out as for icp_frame_end.
 * ICP_ERR_INVALID_ARGUMENT with a message, the context usable as before: a context whose cost is point-to-point, an exchange or
 * profiling switched on, a context held by a batch, a kd-tree sequence (icp_odometry_init) on the same context, a launch before
 * icp_pmap_odometry_init or while a frame awaits its end, an end with nothing launched, n != H*W (or host memory, timestamps, a
 * grid sample) for a vertex map, normals_kernel_size not odd in 1..15.
 * A frame without a single valid target (an all-null vertex map) is no error: as in icp_pmap_register, the residual-norm guard of
 * the Gauss-Newton step (slam/common/optimization.py:323-327) ends its loop in the first iteration with ICP_OK and the guess
 * unchanged, and the frame is completed with that pose.  ICP_ERR_INVALID_JACOBIAN needs rows: a few of them, |det H| < 1e-7.
 * The kind of frame loop is chosen for the life of the context: only icp_destroy ends a kd-tree sequence, so a context that has
 * seen icp_odometry_init refuses these calls from then on (also one that called it between icp_pmap_odometry_init and frame 0,
 * while the projective map was still empty), and a context that holds a projective map refuses icp_odometry_init. */
typedef enum { ICP_FRAME_ROWS = 0, ICP_FRAME_VERTEX_MAP = 1 } icp_frame_layout;
typedef struct icp_pmap_frame_config {
    double voxel_size;           /* > 0: GridSample (slam/preprocessing.py:207-226) in front of the frame (rows input only) */
    float threshold_trans;       /* key-frame test, metres (icp_odometry.py:29-64: 0.1) */
    float threshold_rot;         /* key-frame test, degrees (0.3) */
    int32_t constant_velocity;   /* 1: initial guess = the last relative pose (slam/initialization.py:103-119); 0: identity */
    int32_t targets;             /* rows input — 0: the frame's rows; 1: the pixels of its vertex map.  Vertex-map input: always
                                    its pixels */
    int32_t normals_kernel_size; /* compute_normal_map's window (ProjectiveLocalMapConfig, local_map.py:91-111): odd, 1..15;
                                    default 5 */
    int32_t copy_cloud;          /* 1: icp_pmap_frame_end will be asked for odometry_pc in host memory: its copy starts in
                                    icp_pmap_frame_launch, beside the registration */
} icp_pmap_frame_config;
void icp_default_pmap_frame_config(icp_pmap_frame_config* cfg);
int icp_pmap_register_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16]);
int icp_pmap_odometry_init(icp_ctx* ctx, const icp_pmap_frame_config* cfg);
int icp_pmap_frame_launch(icp_ctx* ctx, const float* data, int64_t n, int mem, int layout, const double* timestamps,
                          const float init_pose[16]);
int icp_pmap_frame_end(icp_ctx* ctx, icp_frame_result* result, float* odometry_pc_out, int64_t cap, int64_t* rows_out,
                       int out_mem, double* loss_per_iter_out, float* dx_per_iter_out);

/* ---- ... for B sequences per call ------------------------------------------------------------------------------------------
 * icp_pmap_frame_launch / icp_pmap_frame_end for the members of a batch, as icp_batch_frame_launch / icp_batch_frame_end are
 * for the kd-tree style map: the projective frame loop (icp_odometry.py:157-246, :360-380; local_map.py:113-235) of B drives
 * behind two calls.  Per member the calls give what the single calls give on that member's context alone with the same frames,
 * bit for bit: pose, parameters, iteration count, losses, steps, key-frame decision, samples, odometry_pc, window, model and
 * every later frame.  One small kernel of its own (the transposition of B vertex maps in one launch).
 *   icp_batch_pmap_odometry_init  icp_pmap_odometry_init(member, cfg) on every member, every member checked before any is
 *                      restarted.  The sequence state is the MEMBER's: a member may be stepped by the batch, then alone with
 *                      icp_pmap_frame_launch / icp_pmap_frame_end, then by the batch again.
 *   icp_batch_pmap_frame_launch  frames[b] = member b's next frame, icp_batch_frame as for icp_batch_frame_launch (`xyz`: the
 *                      rows, or the [3,H,W] vertex map with n = H*W); `mem` and `layout` hold for the whole step.  skip != 0:
 *                      the member sits the step out.  FIRST FRAME (frame index 0): member by member what
 *                      icp_pmap_frame_launch does for frame 0.  REGISTERING (frame index >= 1), ONE call per stage for the whole
 *                      group: the uploads from host arrays (ONE pinned arena, ONE upload stream, two device arenas — those of
 *                      icp_batch_frame_launch), icp_batch_preprocess for a step that grid-samples (rows), icp_batch_project_rows
 *                      (rows; behind the registration for targets = 0) or ONE transposing launch (vertex maps),
 *                      icp_batch_stage, the copies of the staged rows and sample counts on ONE copy stream, and
 *                      icp_batch_pmap_register_launch with every member's guess.
 *   icp_batch_pmap_frame_end  icp_batch_register_end for the registering group, each member's key-frame test, then ONE
 *                      icp_batch_pmap_update over the members whose registration succeeded: the key-frame members pass their
 *                      vertex map, the others NULL.  results, histories, odometry_pc_out / cap / rows_out as for
 *                      icp_batch_frame_end; a skipped member's result is zeroed with frame_index = -1.
 * A FAILED REGISTRATION (ICP_ERR_INVALID_JACOBIAN) leaves its member as icp_pmap_frame_end leaves a single context; every other
 * member completes its frame; the call returns the first such status.  REFUSALS, checked for every member before any member
 * changes (ICP_ERR_INVALID_ARGUMENT, icp_batch_last_error names the member and the reason, "(nothing was changed)"): a
 * non-skipped member without a projective sequence, with a kd-tree sequence, point-to-point, an exchange or profiling, in or
 * awaiting a registration or a frame of its own; a launch while a launch awaits its end; an end with nothing launched; every
 * member skipped; members that differ in voxel_size, targets, normals_kernel_size, image size or stream; for vertex maps
 * n != H*W, host memory, timestamps or a grid sample.  Partial steps run on the inner batches of icp_batch_frame_launch (an LRU
 * of 8 member masks).  A frame the batch has launched is ended by the batch. */
int icp_batch_pmap_odometry_init(icp_batch* batch, const icp_pmap_frame_config* cfg);
int icp_batch_pmap_frame_launch(icp_batch* batch, const icp_batch_frame* frames, int mem, int layout);
int icp_batch_pmap_frame_end(icp_batch* batch, icp_frame_result* results, float* const* odometry_pc_out, const int64_t* cap,
                             int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out);

/* ---- multi-GPU exchange inside the library ("one-shot P2P write+flag all-reduce") -----------------
 * The per-iteration exchange of the scan-sharded registration without leaving the library: after these three calls
 * icp_register / icp_register_launch on every rank enqueue, per ICP iteration, the iteration kernel and ONE kernel that
 * sums this rank's partial rows, writes the 32 doubles into every peer's inbox over xGMI, waits for all ranks'
 * contributions, adds them in rank order and solves — identical poses on all ranks, no host involvement, no RCCL call.
 *   icp_exchange_create  allocates this rank's inbox (uncached device memory) and returns its IPC handle (64 bytes,
 *                        hipIpcMemHandle_t) for the caller to all-gather over its own side channel (torch.distributed
 *                        `all_gather_object`, MPI, a file);
 *   icp_exchange_connect opens the `world` handles (rank order; the own entry is ignored) and switches the context to
 *                        exchange mode; every rank must then issue the same sequence of registrations;
 *   icp_exchange_destroy leaves exchange mode and releases the mappings.
 * All three are refused ("registration in progress") while a registration is in progress, enqueued or uncollected: its
 * iterations were planned with or without the exchange.
 * A peer that does not deliver within the budget (option "exchange_timeout_ms", default 5000) ends the registration
 * with ICP_ERR_EXCHANGE instead of hanging the GPU — and the context LEAVES exchange mode: the ranks' sequence counters
 * and inbox tags may have diverged, so registrations fall back to the rank-local solve until every rank has called
 * icp_exchange_create + icp_exchange_connect again (fresh inboxes, counters at zero).  world <= 16. */
#define ICP_EXCHANGE_HANDLE_BYTES 64
int icp_exchange_create(icp_ctx* ctx, int32_t rank, int32_t world, void* handle_out);
int icp_exchange_connect(icp_ctx* ctx, const void* handles);
int icp_exchange_destroy(icp_ctx* ctx);

/* ---- multi-GPU, map-sharded normal estimation (BASELINE configs[3]: 1M-point map over 8 GPUs) ------
 * KdTreeLocalMap.__get_normals (slam/odometry/local_map.py:397-422) costs O(map) per map update once the map is much
 * larger than the scan.  Every rank keeps the whole map (queries stay local) but estimates only the normals of the points
 * whose 1-metre spatial bucket hashes to it: icp_map_normals_owned fills normals_by_index [M,4] float (device memory of
 * the caller, e.g. a torch tensor; nx, ny, nz, 1 at the ORIGINAL index of every owned point, zeros elsewhere), the
 * caller sums the arrays of all ranks (one RCCL all-reduce: every index has exactly one non-zero contribution, so the
 * sum is exact) and icp_map_normals_install scatters the result into this rank's normal cache, after which
 * registrations run the fused path.  world = 1 reduces to the eager single-GPU estimation (same values). */
int icp_map_normals_owned(icp_ctx* ctx, int32_t rank, int32_t world, float* normals_by_index);
int icp_map_normals_install(icp_ctx* ctx, const float* normals_by_index);
/* Test support for the normal cache (no reference counterpart): the cache of the hash grid as it stands, by ORIGINAL map
 * index, in the layout of icp_map_normals_owned / _install.
 *   normals4_out  [M,4] float32 (M = icp_map_size): (nx, ny, nz, 1) with the bits the cache holds where the point's normal is
 *                 there (estimated, installed, or carried over a pose-only update by option "carry_normals"), four zeros where
 *                 it is not — a point whose normal the next search would estimate on demand
 * Launches nothing: nothing is estimated and no flag changes; it waits for the context's map stream and its own copies, so a
 * map update enqueued before the call is seen complete.  Refused with ICP_ERR_INVALID_ARGUMENT while a registration or a
 * frame is in flight or uncollected (icp_register_end / icp_frame_end first) and with ICP_ERR_EMPTY_MAP on an empty map;
 * icp_last_error says which.  The map, the cache, the NN cache and the registration state are left as they were. */
int icp_map_normals_peek(icp_ctx* ctx, float* normals4_out, int out_mem);

/* ---- aggregated world map: one point per voxel of everything a drive has seen, kept on the device -----------------------
 * The first step of the reference's loop closure (slam/loop_closure.py:272-291: grid-sample every registered cloud, move it
 * by its absolute pose — apply_pose / transform_pointcloud, slam/common/pose.py:40-49 —, concatenate a window of frames,
 * re-express the window in the frame of its middle pose) as a persistent structure fed frame by frame.  A map belongs to
 * the context it was created on: its work is enqueued on that context's stream, its errors are read with icp_last_error
 * of that context, it is destroyed before the context is.  Several maps may live on one context; a map's buffers are its
 * own, so an insert between icp_register_launch and icp_register_end is legal and leaves the registration untouched.
 *   voxel size v > 0, capacity C >= 1 points, at most R >= 1 rows per insert, C + R <= 2^30.
 *   world point  w = ((r0 x + r1 y) + r2 z) + t in float64, every product and sum rounded once; voxel c = rint(w / v),
 *                half to even (the rounding of icp_grid_sample); the voxel key is the three coordinates themselves
 *                (21 bits each): two voxels never merge.
 *   set aside    a row with a non-finite w (counted in nonfinite), else with a coordinate outside [-2^20, 2^20)
 *                (out_of_range): neither touches the map.
 *   creation     a voxel is created by the first insert that reaches it; its point is the w of the row with the smallest
 *                index among that insert's rows in the voxel, its first_frame that insert's frame_id.
 *   updates      every finite in-range row that falls into a stored voxel — the creating insert's rows included — adds 1 to
 *                the voxel's hits (uint32) and raises its last_frame to max(last_frame, frame_id).
 *   order        stored points are numbered insert by insert, within an insert by ascending index of the creating rows.
 *   capacity     of the voxels an insert would create the first ones in that order are stored while there is room; the
 *                others stay unstored for good, and every row that falls into one of them — or, once the map holds C points,
 *                into an unknown voxel — is counted in dropped.  No call fails because the map is full.
 *   table        open addressing over the power of two at or above 2 (C + R) slots, first slot from the mixed key
 *                (x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; slot = x & mask), linear probing; every probe ends
 *                after as many steps as there are slots and sets bit 0 of the error word then.
 *   footprint    24 bytes per slot + 32 per point of C + 16 per row of R (+ 12 per row of R in pinned host memory once
 *                host rows have been inserted). */
typedef struct icp_aggmap icp_aggmap;
typedef struct {
    int64_t size;         /* stored points */
    int64_t inserts;      /* icp_aggmap_insert calls accepted since creation or the last clear */
    int64_t dropped;      /* rows that fell into unstored or (full map) unknown voxels */
    int64_t out_of_range; /* finite rows with a voxel coordinate outside [-2^20, 2^20) */
    int64_t nonfinite;    /* rows whose world point is not finite */
    int64_t error;        /* 0, or bit 0: a probe visited every slot (never seen: the table is at most half full) */
} icp_aggmap_counters;
/* a map for slam/loop_closure.py:272-291 (points moved by slam/common/pose.py:40-49); ICP_ERR_INVALID_ARGUMENT for v <= 0 or
 * non-finite, C < 1, R < 1, C + R > 2^30 */
int icp_aggmap_create(icp_ctx* ctx, double voxel_size, int64_t capacity, int64_t max_insert_rows, icp_aggmap** out);
/* waits for the map's work, then frees it (slam/loop_closure.py:272-291, slam/common/pose.py:40-49: no counterpart) */
void icp_aggmap_destroy(icp_aggmap* map);
/* one registered cloud into the map: slam/loop_closure.py:272-291 per frame — the rows xyz [n,3] float32 moved by the
 * absolute pose [4,4] float64, row-major, as transform_pointcloud does (slam/common/pose.py:40-49), in float64.  Three
 * launches, asynchronous; host rows go through a pinned buffer of the map.  n = 0 counts as an insert and launches nothing.
 * ICP_ERR_INVALID_ARGUMENT, before any launch, for n < 0, n > R, a non-finite pose entry, an unknown memory kind. */
int icp_aggmap_insert(icp_aggmap* map, const float* xyz, int64_t n, int mem, const double pose[16], int32_t frame_id);
/* the counters of the map behind everything enqueued (synchronises): how much of slam/loop_closure.py:272-291's
 * concatenation — clouds moved by slam/common/pose.py:40-49 — the map holds and what it set aside */
int icp_aggmap_stats(icp_aggmap* map, icp_aggmap_counters* out);
/* the stored points in storage order, the concatenation of slam/loop_closure.py:272-291 (clouds moved by
 * slam/common/pose.py:40-49): xyz_out [size,3] = float32(w - origin), subtracted in float64 and rounded once (origin NULL:
 * zero); hits_out [size] uint32; first_frame_out / last_frame_out [size] int32.  Any output may be NULL; `cap` = rows the
 * outputs have room for; *size_out = the map's size (also when ICP_ERR_INVALID_ARGUMENT says cap is below it).  Synchronises. */
int icp_aggmap_get(icp_aggmap* map, const double origin[3], float* xyz_out, uint32_t* hits_out, int32_t* first_frame_out,
                   int32_t* last_frame_out, int64_t cap, int out_mem, int64_t* size_out);
/* ... the float64 world points w themselves [size,3] (slam/loop_closure.py:272-291, slam/common/pose.py:40-49) */
int icp_aggmap_get_f64(icp_aggmap* map, double* xyz_out, int64_t cap, int out_mem, int64_t* size_out);
/* the window of slam/loop_closure.py:272-291 (its lines :287-291): the stored points with frame_lo <= first_frame < frame_hi, in
 * storage order, moved by `pose` [4,4] float64 — the inverse of the window's middle pose — with the float64 arithmetic of the
 * insert (slam/common/pose.py:40-49) and rounded once to float32: xyz_out [count,3], index_out [count] int32 = their stored
 * indices; `cap` = rows the outputs have room for; *count_out = rows of the window (also when ICP_ERR_INVALID_ARGUMENT says
 * cap is below it).  ICP_ERR_INVALID_ARGUMENT for frame_lo > frame_hi, a non-finite pose entry, an unknown memory kind.
 * Synchronises. */
int icp_aggmap_submap(icp_aggmap* map, int32_t frame_lo, int32_t frame_hi, const double pose[16], float* xyz_out,
                      int32_t* index_out, int64_t cap, int out_mem, int64_t* count_out);
/* empties the map and keeps its memory (a new window of slam/loop_closure.py:272-291, slam/common/pose.py:40-49); asynchronous */
int icp_aggmap_clear(icp_aggmap* map);

/* ---- elevation image: a cloud rasterised top-down, the highest point per pixel ------------------------------------------
 * ElevationImageRegistration.build_image of the reference (slam/common/registration.py:196-241), which its loop closure calls
 * on every aggregated window (slam/loop_closure.py:294) and its elevation-image initialisation on every raw scan
 * (slam/initialization.py:176).  An image belongs to the context it was created on, like an aggregated map: its work goes on
 * that context's stream, its buffers are its own (a build between icp_register_launch and icp_register_end is legal and leaves
 * the registration untouched), it is destroyed before the context is.  Several images may live on one context.
 *   pixel      row = rint(x / pixel_size + H / 2), column = rint(y / pixel_size + W / 2), half to even, in the type of the
 *              rows: for float32 rows pixel_size is rounded to float32 and division and sum are float32 operations, for
 *              float64 rows everything is float64.  H / 2, W / 2: floor divisions.  A row is in the image iff
 *              0 <= row < H and 0 <= column < W; a NaN or infinite x or y is outside.
 *   height     z clipped to [z_min, z_max], the bounds rounded to the rows' type (+-inf clip like any value), -0.0 made +0.0.
 *              The pixel goes to the greatest clipped z, with `flip` to the smallest.  Among rows of EQUAL clipped z the
 *              highest row index wins, flipped or not (the reference leaves ties to an unstable sort: it has no rule).
 *   theta      (clipped z - z_min) / (z_max - z_min): the denominator subtracted in float64 and rounded to the rows' type,
 *              subtraction and division in the rows' type, stored as float32.  An empty pixel holds float32(z_min), not 0.
 *   colour     `lut` [259,3] uint8 = 256 colours, then the under, over and bad colour (for a matplotlib colour map
 *              uint8(lut[:, :3] * 255.0)); its row is matplotlib's for a float32 image: t = theta * 256 in float32, t == 256
 *              becomes 255; NaN: 258, t < 0: 256, t >= 256: 257, else trunc(t).
 *   outputs    rgb [H,W,3] uint8; theta [H,W] float32; points [H,W,3] float32: the winning row rounded once to float32, zeros
 *              where the pixel is empty (`points_3D`); index [H,W] int32: the winning row, -1 where empty (`pc_indices`).
 *   deviation  a row in the image whose z is NaN is set aside and counted in rows_nan_z; in the reference it wins its pixel
 *              (argsort puts NaN last, the order is then reversed) and paints it with the bad colour.
 *   launches   clear, splat, resolve on the context's stream, no host read: float32 rows are splat in one pass (64-bit
 *              atomic maximum of the ordered bits of the clipped z above the row), float64 rows and map windows in two (the
 *              extreme z of the pixel, then the highest row among the rows that have it).
 *   footprint  35 bytes per pixel + 9 KB + 24 per row of max_rows (and as much pinned host memory) once host rows have been built
 *              from. */
typedef struct icp_elevation icp_elevation;
typedef enum { ICP_ELEVATION_F32 = 0, ICP_ELEVATION_F64 = 1 } icp_elevation_dtype;
typedef struct {
    int64_t rows_in_image; /* rows of the last build inside the image with a z that is no NaN */
    int64_t rows_outside;  /* rows outside the image (a NaN or infinite x or y among them) */
    int64_t rows_nan_z;    /* rows inside the image set aside for a NaN z */
    int64_t filled_pixels; /* pixels that hold a row */
} icp_elevation_counters;
/* an image object for slam/common/registration.py:196-241 with the settings of its constructor (:185-194): H x W pixels of
 * pixel_size, the clip range, flip_z_axis, the colour table [259,3] uint8 in host memory (copied), at most max_rows rows a
 * build.  ICP_ERR_INVALID_ARGUMENT for a pixel_size that is not positive and finite, a non-finite bound, z_min >= z_max (also
 * once rounded to float32), H < 1, W < 1, H x W > 2^31 - 1, max_rows < 1 or > 2^31 - 1, a NULL table. */
int icp_elevation_create(icp_ctx* ctx, int64_t height, int64_t width, double pixel_size, double z_min, double z_max, int flip,
                         const uint8_t* lut, int64_t max_rows, icp_elevation** out);
/* waits for the image's work, then frees it (slam/common/registration.py:196-241: no counterpart) */
void icp_elevation_destroy(icp_elevation* img);
/* slam/common/registration.py:196-241 on the rows xyz [n,3] of `dtype` (icp_elevation_dtype), as slam/initialization.py:176
 * calls it on a raw scan: asynchronous, three launches (float64 rows: four); host rows go through a pinned buffer of the
 * image, device rows are read in place and must stay untouched until the stream has passed the build.  n = 0 builds the
 * empty image.  ICP_ERR_INVALID_ARGUMENT, before any launch, for n < 0, n > max_rows, n > 2^31 - 1, an unknown memory kind
 * or dtype. */
int icp_elevation_build(icp_elevation* img, const void* xyz, int64_t n, int mem, int dtype);
/* slam/common/registration.py:196-241 as slam/loop_closure.py:294 calls it, on the window of slam/loop_closure.py:287-291
 * without materialising it: the stored points of `map` with frame_lo <= first_frame < frame_hi, each moved by `pose` [4,4]
 * float64 with the arithmetic of icp_aggmap_submap, splat as float64 rows.  index = the stored index; points = the moved point
 * rounded once to float32 — for every filled pixel the row icp_aggmap_submap returns for that stored index, bit for bit.
 * Asynchronous, four launches, the map's size is read on the device.  ICP_ERR_INVALID_ARGUMENT, before any launch, for a map
 * of another context, frame_lo > frame_hi, a non-finite pose entry. */
int icp_elevation_build_aggmap(icp_elevation* img, icp_aggmap* map, int32_t frame_lo, int32_t frame_hi, const double pose[16]);
/* what slam/common/registration.py:196-241 returns, of the last build: rgb_out [H,W,3] uint8 (:229-230), theta_out [H,W] float32
 * (:227-228), points_out [H,W,3] float32 (:233-236), index_out [H,W] int32 (:238-239).  Any output may be NULL.  Copies to host
 * or device memory behind the build; synchronises only for host outputs.  ICP_ERR_INVALID_ARGUMENT for an unknown memory kind. */
int icp_elevation_get(icp_elevation* img, uint8_t* rgb_out, float* theta_out, float* points_out, int32_t* index_out, int out_mem);
/* the counters of the last build (synchronises): what slam/common/registration.py:196-241 kept (:205), dropped and painted */
int icp_elevation_stats(icp_elevation* img, icp_elevation_counters* out);

/* ---- cloud-to-cloud refinement: point-to-point ICP of one cloud against another ------------------------------------------
 * ElevationImageLoopClosure._compute_transform of the reference (slam/loop_closure.py:210-225, called at :237-243 on the
 * `points_3D` of a candidate image and of the current one): Open3D's registration_icp with TransformationEstimationPointToPoint,
 * a distance threshold of 1.0 m, at most 30 iterations, relative_fitness = relative_rmse = 1e-6.  A refiner belongs to the
 * context it was created on, like an aggregated map or an elevation image: its work goes on that context's stream, its buffers
 * and its search grid are its own (every call is legal between icp_register_launch and icp_register_end and inside a frame
 * call, and leaves the map, the grid, the normals, the nearest-neighbour cache and the registration state untouched), it is
 * destroyed before the context is.  Several refiners may live on one context.
 *   rows        float32 [n,3].  A target row with a NaN or infinite coordinate is never matched; a source row with one has no
 *               correspondence and counts in the fitness denominator.  Under ICP_REFINE_DROP_ZERO_ROWS a row of either cloud
 *               whose float32 (x*x + y*y) + z*z is not > 0 is left out altogether — not matched, not counted, in no sum: the
 *               reference's `norm > 0` filter (:238-241), so that an [H,W,3] points_3D image can be passed as it is.
 *               Correspondences always name ORIGINAL target rows.
 *   transform   T float64 [4,4], source into target, starts as `init`.  A moved point is p'_a = ((T_a0 x + T_a1 y) + T_a2 z) +
 *               T_a3 on the float32 coordinates converted to float64, always from the ORIGINAL row, without contraction.
 *   search      over the target rows q: d2 = (dx dx + dy dy) + dz dz in float64, dx = p'_x - (double)q_x; q is a candidate iff
 *               d2 < max_distance * max_distance (the float64 product; strict, as the bound of icp_knn_query); the winner is the
 *               smallest (d2, target row): exact ties go to the lower row.  No result depends on cell_size.
 *   evaluation  fitness = correspondences / counted source rows, inlier_rmse = sqrt(sum d2 / correspondences); both 0 without
 *               correspondences.
 *   step        Umeyama without scaling over the correspondences: means mu_p, mu_q, H = sum (q - mu_q)(p' - mu_p)^T / n,
 *               H = U S V^T, R = U diag(1, 1, sign(det U det V)) V^T, t = mu_q - R mu_p; the identity without a correspondence;
 *               T <- update T as a plain float64 4 x 4 product.  R is computed as the unit quaternion of the greatest eigenvalue
 *               of Horn's 4 x 4 matrix of H (Jacobi rotations): the same rotation where it is unique, a proper rotation always.
 *   loop        evaluate at init; then up to max_iteration times: step, evaluate, stop when |fitness - previous| <
 *               relative_fitness and |inlier_rmse - previous| < relative_rmse.  max_iteration = 0 evaluates only.
 *   history     for every evaluation the T it ran with and 17 figures: count, sum d2, mu_p [3], mu_q [3], H [9] row-major.
 *   deviations  Open3D moves its copy of the source incrementally by every update (the rounding of 30 moves piles up in the
 *               points); here every iteration moves the original row by the accumulated T.  Open3D's kd-tree leaves ties to its
 *               traversal order; here the lower row wins.  Open3D's Eigen SVD and the quaternion differ in the last bits, and
 *               on degenerate correspondences (fewer than 3, a line, one target row) in the rotation they pick.
 *   range       target rows whose cell floor(x / cell_size) leaves [-2^20, 2^20) on an axis are left unmatched and raise a
 *               flag on the device; icp_refine_end reads it and returns ICP_ERR_INVALID_ARGUMENT beside the filled result.
 *               max_distance above 7 cells is searched exhaustively (every target row for every source row).
 *   launches    icp_refine_set_target: clear, count, scan, scatter — a hashed uniform grid over the target with verified 64-bit
 *               cell keys.  icp_refine_launch: max_iteration + 1 pairs of (fused move + search + reduce, one-workgroup solve);
 *               once the loop has stopped on the device the remaining launches return at their first instruction.  No host
 *               read before icp_refine_end, no float atomics: two runs of one call are bit-equal in every output.
 *   footprint   24 bytes per target row + 16 per table slot (the power of two >= 2 max_target_rows, >= 64) + 4 per source row +
 *               about 600 KB; + 12 per row of a cloud (and as much pinned host memory) once it has been given from host memory. */
typedef struct icp_refine icp_refine;
#define ICP_REFINE_DROP_ZERO_ROWS 1
typedef struct {
    double max_distance;     /* correspondence bound in metres (icp_distance_threshold) */
    double relative_fitness; /* stop test on |fitness - previous fitness| */
    double relative_rmse;    /* ... and on |inlier_rmse - previous inlier_rmse| */
    int32_t max_iteration;   /* 0..1000 steps */
    int32_t flags;           /* ICP_REFINE_DROP_ZERO_ROWS for the SOURCE rows */
} icp_refine_params;
typedef struct {
    double transformation[16];    /* T [4,4] row-major, source into target (the reference's caller inverts it) */
    double fitness, inlier_rmse;  /* of the last evaluation, which ran with T */
    int64_t correspondences;      /* ... and its number of matched source rows */
    int64_t source_rows;          /* counted source rows: the fitness denominator */
    int64_t target_rows;          /* target rows that were not left out */
    int64_t source_rows_left_out; /* rows ICP_REFINE_DROP_ZERO_ROWS took from the source */
    int64_t target_rows_left_out; /* ... and from the target */
    int32_t iterations;           /* steps taken */
    int32_t converged;            /* 1: the stop test ended the loop, 0: max_iteration did */
} icp_refine_result;
/* the settings of the reference's call at slam/loop_closure.py:210-225: 1.0, 1e-6, 1e-6, 30 iterations, no flag */
void icp_default_refine_params(icp_refine_params* params);
/* a refiner for slam/loop_closure.py:210-225 with room for max_target_rows and max_source_rows rows and a search grid of
 * cell_size metres (a matter of speed alone; the reference's bound, 1.0, is a good edge).  ICP_ERR_INVALID_ARGUMENT for a
 * cell_size that is not positive and finite, a capacity < 1 or > 2^31 - 1, a NULL `out`. */
int icp_refine_create(icp_ctx* ctx, int64_t max_target_rows, int64_t max_source_rows, double cell_size, icp_refine** out);
/* waits for the refiner's work, then frees it (slam/loop_closure.py:210-225: no counterpart) */
void icp_refine_destroy(icp_refine* refiner);
/* the `target` cloud of slam/loop_closure.py:210-225: xyz [n,3] float32, `flags` ICP_REFINE_DROP_ZERO_ROWS or 0.  Asynchronous,
 * four launches; host rows are copied into a pinned buffer of the refiner before the call returns, device rows are read in place and must stay untouched until the
 * stream has passed the build.  n = 0 is legal (nothing matches).  ICP_ERR_INVALID_ARGUMENT, before any launch, for n < 0,
 * n > max_target_rows, an unknown memory kind or flag, a refinement in flight. */
int icp_refine_set_target(icp_refine* refiner, const float* xyz, int64_t n, int mem, int32_t flags);
/* the registration_icp call of slam/loop_closure.py:210-225 on the `source` cloud xyz [n,3] float32 from `init` [4,4] float64
 * (row-major): enqueues the whole loop and returns.  Device rows must stay untouched until icp_refine_end.  n = 0 is legal:
 * fitness 0, inlier_rmse 0, 0 iterations, the transformation equals init.  ICP_ERR_INVALID_ARGUMENT, before any launch, for
 * n < 0, n > max_source_rows, an unknown memory kind or flag, a max_distance that is not positive and finite (or whose square is
 * not), max_iteration outside 0..1000, a negative threshold, a non-finite init entry, no target set, a refinement in flight. */
int icp_refine_launch(icp_refine* refiner, const float* xyz, int64_t n, int mem, const double init[16], const icp_refine_params* params);
/* waits for the refinement and returns what registration_icp does at slam/loop_closure.py:210-225 (`result` may be NULL);
 * correspondence_out [n] int32 (host or device memory, may be NULL): the target row of every source row at the last evaluation,
 * -1 without one.  ICP_ERR_INVALID_ARGUMENT with nothing launched, for an unknown memory kind, and — behind the filled result —
 * when target rows lay outside +-2^20 cells. */
int icp_refine_end(icp_refine* refiner, icp_refine_result* result, int32_t* correspondence_out, int out_mem);
/* the rows of an elevation image for slam/loop_closure.py:210-225, IN PLACE: *xyz_out = the device pointer of the image's
 * `points_3D` [H * W,3] float32, *n_out = H * W, to be passed on to icp_refine_set_target / icp_refine_launch as device memory
 * with ICP_REFINE_DROP_ZERO_ROWS (empty pixels are all-zero rows).  No copy and no launch; the image must not be rebuilt or
 * destroyed before the stream has passed the target build, or, for a source, before icp_refine_end.
 * ICP_ERR_INVALID_ARGUMENT for a NULL image or output, an image of another context. */
int icp_refine_image_rows(icp_refine* refiner, icp_elevation* image, const float** xyz_out, int64_t* n_out);
/* the evaluations of the refinement icp_refine_end collected last (slam/loop_closure.py:210-225: Open3D keeps none):
 * transforms_out [iterations + 1,16] and sums_out [iterations + 1,17] float64 in host memory, either may be NULL; `cap` = rows
 * the outputs have room for.  ICP_ERR_INVALID_ARGUMENT for cap < iterations + 1 or before any icp_refine_end.  Synchronises. */
int icp_refine_history(icp_refine* refiner, double* transforms_out, double* sums_out, int32_t cap);

/* ---- profiling hooks ---------------------------------------------------------------------------------------------
 * Accumulated HIP-event time (ms) and launch count of the dominant kernel (the per-iteration nearest-neighbour
 * search) since the last reset; measured on the context's stream.  `enable` is a bit mask: 1 = search kernel,
 * 2 = reduction, 4 = normal estimation (0 disables). */
int icp_profile_enable(icp_ctx* ctx, int enable);
int icp_profile_read(icp_ctx* ctx, double* search_ms_out, int64_t* search_launches_out, double* reduce_ms_out,
                     double* normals_ms_out);
/* the search kernel's time by ICP iteration index: ms_out / launches_out [cap] (index cap - 1 and beyond: not reported
 * separately beyond 64).  With the option "profile_rotate" 1 only ONE iteration launch per registration is bracketed —
 * iteration (number of the registration) mod max_num_alignments — so that every frame of a run can be sampled at the cost
 * of two event records, and every iteration index is seen equally often. */
int icp_profile_read_iterations(icp_ctx* ctx, double* ms_out, int64_t* launches_out, int32_t cap);
/* what an event pair ADDS to the launch it brackets, on the context's stream (median of `samples`, microseconds): the
 * pair is put around a kernel that spins for exactly 20 us of the device's wall clock, with a busy predecessor and a
 * successor like a launch inside a registration has them; the result is the measured time minus those 20 us — the dispatch
 * latency behind the barrier packet of the first event, which back-to-back launches do not pay and rocprofv3's kernel
 * durations do not contain.  bench.py subtracts it from its live event timing of the dominant kernel. */
int icp_profile_event_floor(icp_ctx* ctx, int32_t samples, double* median_us_out);

#ifdef __cplusplus
}
#endif
#endif /* ICP_MI355X_H */
