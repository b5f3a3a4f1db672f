/*
 * kmx_abi.h — the C ABI of the MI355X-native dpgo / Kimera-Multi-LCD hot path.
 *
 * This is the drop-in boundary. Every entry point replaces the
 * bottom of one reference interface. The reference sources are NOT vendored in
 * /root/reference (SURVEY.md §0 finding 1); the interfaces are cited from the
 * fork author's call-flow diagram `images/kimera-multi.drawio` (drawio:N) and the
 * in-tree parameter files.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every function returns int: 0 = ok, < 0 = error (KMX_E*). kmx_last_error()
 *     returns a thread-local message for the last failing call.
 *   - Host arrays are owned by the caller and only read/written during the call.
 *     Device buffers are owned by the handle, except the exchange buffers of
 *     kmx_pgo_pack_public / kmx_pgo_unpack_public, which are caller-owned device
 *     pointers (e.g. torch tensors used with RCCL).
 *   - A handle is not thread-safe. All of its device work is enqueued on one HIP
 *     stream (its own, or the caller's via kmx_pgo_set_stream); calls that return
 *     host data synchronise that stream.
 *   - Lifted pose layout: pose i of a robot block is X_i = [Y_i p_i] in
 *     R^{r x (d+1)}, stored row-major: X[i*4r + a*4 + c], a < r, c < 4 (c = 3 is p).
 *     d = 3 is fixed.
 */
#ifndef KMX_ABI_H
#define KMX_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMX_ABI_VERSION 10

/* error codes */
#define KMX_OK 0
#define KMX_EINVAL (-1)   /* bad argument / shape */
#define KMX_EHIP (-2)     /* HIP runtime error */
#define KMX_ESTATE (-3)   /* call out of order (e.g. iterate before set_graph) */
#define KMX_ENOMEM (-4)
#define KMX_EUNSUP (-5)   /* unsupported parameter value (e.g. relaxation rank), or an
                              input past a fixed capacity (kmx_bow_query: tied scores) */
#define KMX_ETIMEOUT (-6) /* a bounded wait expired (kmx_pgo_sync_timeout)       */

const char* kmx_last_error(void);
int kmx_abi_version(void);
/* number of visible HIP devices (0 when no GPU). Does not create a context. */
int kmx_device_count(int* out);

/* ------------------------------------------------------------------------- */
/* dpgo: distributed pose-graph optimisation (RBCD on lifted SE(3) with GNC)  */
/* ------------------------------------------------------------------------- */

/* Robust cost selector. Reference: dpgo RobustCostType, selector `GNC_TLS`
 * (drawio:2175). Only L2 and GNC_TLS are on the hot path. */
#define KMX_COST_L2 0
#define KMX_COST_GNC_TLS 1

/* Local solver of a block update (dpgo ROptParameters::ROptMethod). */
#define KMX_METHOD_RTR 0 /* Riemannian trust region + truncated CG (the default) */
#define KMX_METHOD_RGD 1 /* one preconditioned Riemannian gradient step, fixed step size */

/* Block-update schedule across robots (SURVEY.md §0 finding 6). */
#define KMX_SCHEDULE_SEQUENTIAL 0 /* one executing robot per round (dpgo_ros sync) */
#define KMX_SCHEDULE_CONCURRENT 1 /* every active robot per round (Jacobi)        */

/* Mirrors dpgo PGOAgentParameters + ROptParameters + RobustCostParameters
 * (drawio:2457-2513). Values in comments are the defaults kmx.dpgo uses. */
typedef struct kmx_pgo_params {
  int d;                    /* 3 (only 3 is supported)                        */
  int r;                    /* relaxation rank, 3..8 (5)                      */
  int rtr_iterations;       /* RTR outer iterations per block update (1)      */
  int tcg_max_iterations;   /* truncated-CG inner iterations (10)             */
  double tcg_kappa;         /* tCG linear-convergence target (0.1)            */
  double tcg_theta;         /* tCG superlinear exponent (1.0)                 */
  double rtr_initial_radius;/* trust radius at the start of a block update (100) */
  double rtr_max_radius;    /* (1e4)                                          */
  double rtr_accept_rho;    /* accept the step if rho > this (0.1)            */
  double gradnorm_tol;      /* skip the block update if ||grad|| < tol (1e-2) */
  int use_preconditioner;   /* block-Jacobi preconditioner on/off (1)         */
  double precond_shift;     /* lambda added to each 4x4 diagonal block (1e-1) */
  int robust_cost;          /* KMX_COST_* (GNC_TLS)                           */
  double gnc_barc;          /* TLS error threshold c-bar (5.0)                */
  double gnc_mu_init;       /* GNC initial mu (1e-5)                          */
  double gnc_mu_step;       /* mu <- mu * step after each weight update (1.4) */
  int acceleration;         /* Nesterov-accelerated RBCD (RBCD++) on/off (0); concurrent
                               schedule only: every local robot updates every round      */
  int restart_interval;     /* acceleration restart period in rounds (30)               */
  int method;               /* KMX_METHOD_RTR (0) or KMX_METHOD_RGD (1)                  */
  int tcg_form;             /* KMX_TCG_FORM_STANDARD (0): ROPTLIB's tCG, two dependent
                               reductions per step; KMX_TCG_FORM_ONESYNC (1): opt-in, one
                               reduction and one kernel per step, the
                               neighbours' new direction formed from gathered z, M^-1 H delta
                               and delta; parity with the standard form at convergence only
                               (2, ABI 7's persistent resident round, was removed in ABI 8:
                               level with these forms)              */
  double rgd_stepsize;      /* RGD: X <- Retr_X(-s * precon(grad f)) (1e-3)              */
  int tile_incidences;      /* incidences per workgroup tile (0: from the handle's local
                               problem, 180..2 chunks; the tile cut orders the per-robot
                               reductions, so handles that must agree bit for bit across
                               placements set the same value)                            */
  int reserved;
} kmx_pgo_params;

/* Per-robot statistics of one RBCD round (what dpgo logs to dpgo_log_*.csv via
 * logIteration, drawio:2136-2142).
 * A block update runs rtr_iterations RTR iterations; one whose gradient norm is
 * below gradnorm_tol is skipped and ends the block update (tcg_stop =
 * KMX_TCG_SKIPPED, tcg_iterations = 0, accepted = 0). rho and radius are those
 * of the last RTR step that was taken in this block update, also when a later
 * iteration was skipped; when the first iteration is skipped no step was
 * taken: rho = 0 and radius = rtr_initial_radius (likewise for RGD, which has
 * no trust region). rel_change is over the whole block update, whatever the
 * number of iterations. */
typedef struct kmx_iter_stats {
  int updated;          /* 1 if this robot executed a block update this round  */
  int tcg_iterations;   /* inner iterations of the last RTR iteration          */
  int tcg_stop;         /* KMX_TCG_*                                           */
  int accepted;         /* last RTR step accepted                              */
  double f_init;        /* local cost before the update                        */
  double gradnorm_init; /* Riemannian gradient norm before the update          */
  double f_final;       /* local cost after the update                         */
  double rho;           /* actual / predicted decrease of the last RTR step    */
  double radius;        /* trust radius after the last RTR step                */
  double rel_change;    /* ||X_new - X_old||_F / sqrt(n) (dpgo relativeChange) */
  int64_t edges;        /* edges in the block's local problem (metric unit)    */
  int64_t hessvecs;     /* Hessian-vector products evaluated                   */
} kmx_iter_stats;

#define KMX_TCG_FORM_STANDARD 0
#define KMX_TCG_FORM_ONESYNC 1

#define KMX_TCG_NONE 0
#define KMX_TCG_NEGATIVE_CURVATURE 1
#define KMX_TCG_EXCEEDED_TR 2
#define KMX_TCG_LINEAR 3      /* ||r|| <= ||r0|| kappa        */
#define KMX_TCG_SUPERLINEAR 4 /* ||r|| <= ||r0||^(1+theta)    */
#define KMX_TCG_MAX_ITER 5
#define KMX_TCG_SKIPPED 6     /* gradient below tolerance: no step */

typedef struct kmx_pgo kmx_pgo;

/* Replaces `PGOAgent(id, PGOAgentParameters)` (drawio:1943-1957, 2457).
 * `device` is the HIP ordinal used by this handle. */
int kmx_pgo_create(const kmx_pgo_params* params, int device, kmx_pgo** out);
int kmx_pgo_destroy(kmx_pgo* h);
/* Use the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream). */
int kmx_pgo_set_stream(kmx_pgo* h, void* hip_stream);

/* How the host enqueues the tCG steps of a round (dpgo's tCG loop inside
 * PGOAgent::iterate, drawio:2058-2066; the results are identical in every mode):
 *   1  polled: after each step the host waits for the device's progress word
 *      and stops enqueueing once every robot left tCG;
 *   0  blind: all tcg_max_iterations steps are enqueued; the kernels of a
 *      finished robot exit at once; the host never waits inside a round;
 *  -1  adaptive (default): a polled loop that needed nearly tcg_max steps sends
 *      the next loops blind, then one polled loop measures again.
 * The environment variable KMX_POLL=0/1 at handle creation forces 0 / 1. */
int kmx_pgo_set_tcg_poll(kmx_pgo* h, int mode);

/* Robot groups of a round. Between the round-begin launch and the final commit
 * a robot's block update reads its own rows and the public table only, so the
 * handle cuts its local robots into contiguous groups of about equal incidence
 * counts and runs each group's launches on a stream of its own (forked after
 * the round begin, joined before the commit; the results are bitwise those of
 * one group). In effect for the launched-reduction form (more than 80k local
 * poses, or KMX_RED=0) with RTR in the standard tCG form and timing off.
 * KMX_TCG_GROUPS=1/2/4 at handle creation sets the number asked for (default
 * 2), clamped to the local robots that have poses.
 * *groups: the groups the next round runs with (1: a single launch chain).
 * bounds (may be NULL, else 5 entries): the cut of the current graph, whether
 * in effect or not: group g holds the local robots [bounds[g], bounds[g + 1])
 * (indices into the handle's local robots in team order); entries past the
 * last group repeat the local robot count. */
int kmx_pgo_get_tcg_groups(kmx_pgo* h, int* groups, int32_t* bounds);

/* The reduction form of the next round's launch chains (additive to ABI 10):
 * 0 launched (a k_reduce launch after every producing kernel), 2 consumer (the
 * next kernel of the chain reduces its robot's partials itself; no k_reduce in
 * a round). Where robot groups are in effect this is the grouped round's form:
 * KMX_GROUP_RED=0/2 at handle creation, by default 2 while no local robot has
 * more than 384 tiles and 0 above that; otherwise the single chain's form
 * (KMX_RED, or by the local pose count). The results are bitwise the same in
 * either form. */
int kmx_pgo_get_group_reduction(kmx_pgo* h, int* form);

/* Native team exchange over RCCL (replaces the ROS topics public_poses +
 * status of dpgo_ros, drawio:2340-2375, for a team with one process per GPU).
 * Rank 0 calls kmx_comm_unique_id and hands the KMX_COMM_ID_BYTES bytes to
 * every rank (any side channel); every rank calls kmx_pgo_comm_init on its
 * handle after kmx_pgo_set_graph, then kmx_pgo_set_exchange with the slot
 * lists of kmx_pgo_exchange_pack / _unpack (host arrays: send_slots grouped by
 * destination rank, recv_slots by source rank, counts[world] each; the own
 * rank's counts equal). From then on every kmx_pgo_iterate /
 * kmx_pgo_iterate_async round starts with the exchange on the handle's stream:
 * gather, one ncclSend / ncclRecv per peer in one group, scatter (rows into the
 * public table, the peers' status words into the team status). Every rank must
 * run the same number of rounds. kmx_pgo_set_graph drops the exchange lists. */
#define KMX_COMM_ID_BYTES 128
int kmx_comm_unique_id(void* out, int64_t nbytes);
/* JSON text: the shared objects libkmx's RCCL and HIP calls resolve to in this
 * process (dladdr of ncclSend / hipMalloc), ncclGetVersion, the RCCL header
 * version kmx was built with, hipRuntimeGetVersion / hipDriverGetVersion. */
int kmx_runtime_info(char* out, int64_t nbytes);
/* The communicator is created non-blocking: a rank whose peers do not all
 * arrive within timeout_s seconds aborts it and returns KMX_EHIP, so one
 * failing rank cannot strand the others in the rendezvous. */
int kmx_pgo_comm_init(kmx_pgo* h, const void* unique_id, int world, int rank, double timeout_s);
/* Drop the communicator and the exchange lists (back to caller-driven
 * exchanges, e.g. after a failed start-up check on another rank). */
int kmx_pgo_comm_destroy(kmx_pgo* h);
int kmx_pgo_set_exchange(kmx_pgo* h, const int32_t* send_slots, const int64_t* send_counts,
                         const int32_t* recv_slots, const int64_t* recv_counts);
/* One exchange now, outside a round (e.g. before kmx_pgo_update_weights);
 * every rank must call it the same number of times. */
int kmx_pgo_exchange(kmx_pgo* h);

/* Replaces the pose-graph intake `PGOAgent::addMeasurement` ->
 * PoseGraph::addOdometry / addPrivateLoopClosure / addSharedLoopClosure
 * (drawio:2142, 2779-2826). Edges are the GLOBAL measurement list of the team:
 * measurement e goes from pose (r1[e],p1[e]) to (r2[e],p2[e]) with rotation
 * R[9e..9e+8] (row-major) and translation t[3e..3e+2], precisions kappa / tau,
 * weight w and fixedWeight flag (odometry). `local[a]` marks robots whose blocks
 * live on this handle; edges with no local endpoint are dropped. Shared loop
 * closures (r1 != r2) are owned by min(r1, r2) for GNC weights (drawio:2198). */
int kmx_pgo_set_graph(kmx_pgo* h, int n_robots, const int32_t* n_poses,
                      const uint8_t* local, int64_t m, const int32_t* r1,
                      const int32_t* p1, const int32_t* r2, const int32_t* p2,
                      const double* R, const double* t, const double* kappa,
                      const double* tau, const double* weight,
                      const uint8_t* fixed_weight);

/* Replaces `initialize(...)` with an injected initial iterate:
 * X is n_poses[robot] * 4r doubles. get_iterate reads the current block back. */
int kmx_pgo_set_iterate(kmx_pgo* h, int robot, const double* X);
int kmx_pgo_get_iterate(kmx_pgo* h, int robot, double* X);

/* Public-pose exchange (publishPublicPoses -> updateNeighborPoses,
 * drawio:2340-2355). The team's public poses (every endpoint of a shared loop
 * closure) form one global table ordered by (robot, pose); its size is
 * kmx_pgo_public_count. pack writes this handle's OWNED rows
 * [first, first+count) of the table (count * 4r doubles) to a caller device
 * buffer; unpack installs a full table (n_public * 4r doubles, device) as the
 * fixed neighbour poses. refresh_local does pack+unpack in-device for the case
 * where every robot is local. set_neighbor_poses is the host-side variant
 * (updateNeighborPoses with a PoseDict): rows for the given (robot,pose). */
int kmx_pgo_public_count(kmx_pgo* h, int64_t* n_public, int64_t* first_owned,
                         int64_t* n_owned);
int kmx_pgo_pack_public(kmx_pgo* h, void* dev_out);
int kmx_pgo_unpack_public(kmx_pgo* h, const void* dev_table);
int kmx_pgo_refresh_local(kmx_pgo* h);
/* Sparse form of the same exchange (one all-to-all instead of an all-gather):
 * gather_public_rows writes the rows of `n` public slots OWNED by this handle
 * (dev_slots: int32 device array of table slots) to dev_out (n * 4r doubles);
 * scatter_public_rows installs n rows received from peers at the given slots.
 * Only the neighbour rows a handle's shared loop closures reference cross the
 * link; refresh_local fills the owned slots. */
int kmx_pgo_gather_public_rows(kmx_pgo* h, const int32_t* dev_slots, int64_t n, void* dev_out);
int kmx_pgo_scatter_public_rows(kmx_pgo* h, const int32_t* dev_slots, int64_t n, const void* dev_rows);
/* The same exchange with the team status piggy-backed (dpgo Status message,
 * drawio:2375, used by shouldUpdateMeasurementWeights' "all agents converged"):
 * the rows are cut into n_seg per-peer segments, segment k = rows
 * [seg[k], seg[k+1]) (dev_seg: n_seg + 1 int32, device), and each segment is
 * followed by ONE double, so segment k starts at double seg[k]*4r + k. pack
 * writes this handle's largest relative change (of its robots' last block
 * updates) after every segment; unpack installs the rows and keeps the n_seg
 * received status values for the next round-begin GNC decision. */
int kmx_pgo_exchange_pack(kmx_pgo* h, const int32_t* dev_slots, int64_t n, const int32_t* dev_seg,
                          int n_seg, void* dev_out);
int kmx_pgo_exchange_unpack(kmx_pgo* h, const int32_t* dev_slots, int64_t n, const int32_t* dev_seg,
                            int n_seg, const void* dev_in);
int kmx_pgo_set_neighbor_poses(kmx_pgo* h, int64_t count, const int32_t* robot,
                               const int32_t* pose, const double* X);
/* The installed public table (n_public * 4r doubles) and, when ext != NULL,
 * the peers' status words of the last exchange (one per per-peer segment):
 * used to check two exchange paths against each other bit for bit. */
int kmx_pgo_get_public(kmx_pgo* h, double* table, double* ext);

/* One RBCD round: `PGOAgent::iterate(doOptimization)` of every robot with
 * active[a] != 0 (drawio:2058-2066, 2513), all using the current neighbour
 * table. stats (may be NULL) receives one record per robot of the team
 * (n_robots records; non-local / inactive robots get updated = 0). */
int kmx_pgo_iterate(kmx_pgo* h, const uint8_t* active, kmx_iter_stats* stats);
/* Enqueue `rounds` concurrent rounds (all local robots active) without any
 * host synchronisation; used by the benchmark. stats are not produced. When
 * refresh_local != 0 the owned public rows are published before the first
 * round (every round republishes the rows it commits): the single-device
 * exchange; otherwise the caller exchanges between rounds. With
 * rtr_iterations > 1 the rows are republished once, at the end of the block
 * update, for every robot one of whose RTR iterations moved its poses, also
 * when its last iteration was rejected or skipped. */
int kmx_pgo_iterate_async(kmx_pgo* h, int rounds, int refresh_local);
/* Acceleration (kmx_pgo_params.acceleration = 1, concurrent schedule only):
 * each round first forms the extrapolated point Y = Proj((1 - alpha) X +
 * alpha V) and sets X := Y (the first of refresh_local / exchange_pack /
 * iterate in a round does it, so the exchanged and published rows are Y and
 * the block update starts from Y); after the block updates V = Proj(V +
 * gamma (X - Y)), and every restart_interval rounds V = X, gamma = 0. Between
 * rounds X is the accelerated iterate itself; between the exchange and
 * iterate it holds Y. set_iterate restarts the acceleration (V = X). */
/* Wait for all work enqueued on the handle's stream. */
int kmx_pgo_sync(kmx_pgo* h);
/* As kmx_pgo_sync with a deadline: KMX_ETIMEOUT when the stream has not
 * drained after timeout_s (a round's exchange waiting on a peer that failed);
 * kmx_pgo_comm_destroy then aborts the communicator, which releases it. */
int kmx_pgo_sync_timeout(kmx_pgo* h, double timeout_s);

/* Diagnostic (no reference counterpart): the phase stamps of the one-sync tCG
 * kernel in a KMX_STEP_STAMPS build (`make -C kimera-multi_amd/csrc stamps`):
 * per tile 16 words — 7 wall-clock stamps (100 MHz; pgo.hip body_step), -,
 * poses, incidences, block index, first tile of its robot — of the last launch
 * that formed step 2. KMX_EUNSUP otherwise. */
int kmx_pgo_debug_step_stamps(uint64_t* out, int64_t n);

/* GNC: `updateMeasurementWeights()` (drawio:2215) for every non-fixed edge with
 * a local endpoint, evaluated at the current iterate and neighbour table, then
 * mu <- mu * mu_step, inner iterations <- 0, updates += 1. mu_out (may be
 * NULL) gets the mu used. A shared loop closure is evaluated identically on
 * the handles of both its robots (same two rows), which yields the owner's
 * weight on both sides (publishMeasurementWeights, drawio:2195-2198). */
int kmx_pgo_update_weights(kmx_pgo* h, double* mu_out);
/* GNC schedule run on the device at the start of every round (iterate and
 * iterate_async) when enabled: shouldUpdateMeasurementWeights
 * (drawio:2466-2469) = GNC_TLS cost, fewer than max_updates updates so far,
 * and (more than inner_iters rounds since the last update, or every agent of
 * the team converged: relative change of its last block update <=
 * rel_change_tol, this handle's robots and the statuses received by
 * kmx_pgo_exchange_unpack). Disabled by default (the agent API decides on the
 * host and calls kmx_pgo_update_weights). */
typedef struct kmx_gnc_state {
  int32_t inner_iter;  /* rounds since the last weight update (dpgo mRobustOptInnerIter) */
  int32_t updates;     /* weight updates so far                                         */
  int32_t last_fired;  /* the last round began with a weight update                      */
  int32_t rounds;      /* rounds completed                                               */
  double mu;           /* GNC mu of the next update                                      */
  double reserved[3];
} kmx_gnc_state;
int kmx_pgo_set_gnc_schedule(kmx_pgo* h, int enabled, int inner_iters, int max_updates,
                             double rel_change_tol);
int kmx_pgo_get_gnc_state(kmx_pgo* h, kmx_gnc_state* out);
int kmx_pgo_set_gnc_state(kmx_pgo* h, const kmx_gnc_state* in);
/* Per-robot relative change of the last block update (dpgo Status
 * relativeChange, drawio:2375; +inf before the first update): n_robots
 * doubles, local robots written/read only. */
int kmx_pgo_get_status(kmx_pgo* h, double* rel_change);
int kmx_pgo_set_status(kmx_pgo* h, const double* rel_change);
int kmx_pgo_get_mu(kmx_pgo* h, double* mu);
int kmx_pgo_set_mu(kmx_pgo* h, double mu);
/* `setMeasurementWeight` (drawio:2268) in bulk: weights indexed by global edge
 * id (m doubles). get returns the weights of edges with a local endpoint (others
 * untouched). set installs all; the handle rebuilds its preconditioner. */
int kmx_pgo_get_weights(kmx_pgo* h, double* w);
int kmx_pgo_set_weights(kmx_pgo* h, const double* w);
/* Shared-edge weight exchange for multi-GPU GNC (owner -> peer, drawio:2198):
 * the team's shared loop closures in global edge order; pack writes owned
 * entries and zeros elsewhere (n_shared doubles, device), unpack installs the
 * all-reduced table. */
int kmx_pgo_shared_count(kmx_pgo* h, int64_t* n_shared);
int kmx_pgo_pack_shared_weights(kmx_pgo* h, void* dev_out);
int kmx_pgo_unpack_shared_weights(kmx_pgo* h, const void* dev_table);

/* Rounded trajectory in the anchor frame: `getTrajectoryInGlobalFrame` /
 * publishTrajectory (drawio:2148-2151) with the global anchor of
 * `setGlobalAnchor` (drawio:2396). anchor = 4r doubles [Y0 p0] (lifted pose of
 * robot 0, pose 0). out: n_poses[robot] * 12 doubles = R (row-major 3x3) then t. */
int kmx_pgo_get_trajectory(kmx_pgo* h, int robot, const double* anchor,
                           double* out);

/* Primitive evaluation for parity tests (one robot block, current neighbour
 * table). mode: KMX_EVAL_*. V/out are n_poses[robot]*4r doubles; scalar gets the
 * cost (COST_EGRAD) or <V, out> otherwise. HESS modes evaluate at the current
 * iterate. */
#define KMX_EVAL_COST_EGRAD 0 /* out = Euclidean gradient at X=V, scalar = f(V) */
#define KMX_EVAL_EHESS 1      /* out = Euclidean Hessian-vector product Q V      */
#define KMX_EVAL_RGRAD 2      /* out = Riemannian gradient at X (V ignored)      */
#define KMX_EVAL_RHESS 3      /* out = Riemannian Hessian at X applied to V      */
#define KMX_EVAL_PRECON 4     /* out = preconditioner at X applied to V          */
#define KMX_EVAL_RETRACT 5    /* out = R_X(V)                                    */
#define KMX_EVAL_PROJECT 6    /* out = Proj(V): the polar factor U V^T of every pose's r x 3
                               * rotation block, translation column unchanged (the projection
                               * of the accelerated rounds; any finite V gives orthonormal
                               * columns, rank-deficient blocks included). Additive to ABI 10. */
int kmx_pgo_eval(kmx_pgo* h, int robot, int mode, const double* V, double* out,
                 double* scalar);

/* Edges in robot `robot`'s local problem (private + shared incident edges). */
int kmx_pgo_local_edges(kmx_pgo* h, int robot, int64_t* m_local);
/* Resident device bytes of the handle and the bytes of one incidence record
 * (68: compact — three components of the rotation's unit quaternion, t,
 * w kappa, w tau with the tail flag in its sign, and the 4-B other endpoint
 * with the fourth component's index; 128: full rotation, when some measurement
 * rotation is not in SO(3) to 1e-12). */
int kmx_pgo_memory(kmx_pgo* h, int64_t* device_bytes, int* record_bytes);
/* Live instrumentation of the dominant kernel (the Hessian-vector product of
 * the tCG loop). When enabled, every Hessian-vector launch enqueued by
 * kmx_pgo_iterate / kmx_pgo_iterate_async is bracketed by a HIP event pair on
 * the handle's stream. read_timing synchronises, sums the event durations and
 * the device-side work counters accumulated since the last read, and resets
 * them. hessvec_alg_bytes follows SURVEY.md §8d: per launch and per robot whose
 * tCG was running, 128 B per local edge + 2 * 8 * r(d+1) B per pose. */
typedef struct kmx_pgo_counters {
  double hessvec_ms_total;     /* summed device time of Hessian-vector launches */
  int64_t hessvec_launches;    /* launches bracketed by events                  */
  double hessvec_alg_bytes;    /* algorithmic bytes those launches processed    */
  int64_t edges_iters;         /* sum over executed block updates of m_alpha    */
  int64_t block_updates;       /* executed block updates (tCG ran)              */
  int64_t hessvecs;            /* robot-level Hessian-vector products           */
  int64_t gnc_updates;         /* GNC weight updates run                        */
} kmx_pgo_counters;
int kmx_pgo_enable_timing(kmx_pgo* h, int enable);
int kmx_pgo_read_counters(kmx_pgo* h, kmx_pgo_counters* out);

/* ------------------------------------------------------------------------- */
/* Kimera-Multi-LCD: descriptor matching + geometric verification             */
/* ------------------------------------------------------------------------- */

#define KMX_NORM_L1 0      /* BruteForce-L1 over bytes: reference build      */
#define KMX_NORM_HAMMING 1 /* BruteForce-Hamming over 256 bits: north_star  */

/* sampler variants of std::uniform_int_distribution<int>(0, INT_MAX) over
 * std::mt19937 (SURVEY.md §0 finding 5) */
#define KMX_RNG_GCC9 0   /* rejection of x >= 2^31, returns x (ROS Noetic)  */
#define KMX_RNG_GCC11 1  /* Lemire: returns x >> 1                          */

/* 5-point minimal solver of the 2D-2D RANSAC (opengv CentralRelativePoseSacProblem). */
#define KMX_ALGO_STEWENIUS 0 /* opengv STEWENIUS: Groebner basis, 10x10 action matrix eigenproblem */
#define KMX_ALGO_NISTER 1    /* opengv NISTER: degree-10 polynomial in z, Sturm roots            */

/* LcdParams (params/D455/LcdParams.yaml:16-17, 51-66). */
typedef struct kmx_lcd_params {
  int norm;                   /* KMX_NORM_* (L1: matcher_type 3 + patch:33-35) */
  double lowe_ratio;          /* 0.7 (compared in double, as LcdParams' double) */
  int min_2d2d_inliers;       /* 10                                            */
  int min_3d3d_inliers;       /* 5                                             */
  double ransac_threshold_2d2d; /* 1e-6 (1 - cos)                              */
  double ransac_threshold_3d3d; /* 0.3 m                                       */
  int ransac_max_iterations;  /* 500                                           */
  double ransac_probability;  /* 0.995                                         */
  int ransac_randomize;       /* 0: fixed seed                                 */
  uint32_t ransac_seed;       /* 12345                                         */
  int rng_variant;            /* KMX_RNG_*                                     */
  int use_1point_3d3d;        /* 1: translation-only 3D-3D given the 2D-2D R   */
  int pose_recovery_type;     /* 0: 3D-3D (reference config), 1: PnP            */
  int min_2d3d_inliers;       /* 20 (LcdParams.yaml:53)                        */
  double ransac_threshold_2d3d; /* PnP inlier threshold in (1 - cos) units: from
                                 a pixel threshold px and focal length f,
                                 1 - cos(atan(px / f)) (LcdParams.yaml:57)     */
  int algorithm_2d2d;         /* KMX_ALGO_* 5-point minimal solver
                                 (ransac_2d2d_algorithm, LcdParams.yaml:73)     */
  int refine_pose;            /* refine_pose (LcdParams.yaml:14): after an accepted
                                 3D-3D recovery (pose_recovery_type 0), T is
                                 re-estimated over all 3D-3D inliers by least
                                 squares (centroids + Kabsch), the restated form
                                 of Kimera-VIO's stereo pose refinement [U]     */
  int rng_stream;             /* LC5, the OpenGV fork's "thread_local" sampler
                                 (README.md:35-36): 0 = every RANSAC problem
                                 seeds its own std::mt19937 with ransac_seed
                                 (opengv's SampleConsensusProblem constructor;
                                 the default); 1 = one engine per verification
                                 thread, seeded once, that every problem
                                 continues in candidate order (2D-2D, then the
                                 Arun / EPnP recovery). Mode 1 is an ordered,
                                 candidate-serial GPU path. */
  int reserved[1];
} kmx_lcd_params;

/* Stages of kmx_lcd_verify_matches. */
#define KMX_LCD_STAGE_2D2D 1    /* geometricVerificationNister (drawio:2589-2592) */
#define KMX_LCD_STAGE_RECOVER 2 /* recoverPose (drawio:2595-2598)                 */

/* computeMatchedIndices (drawio:2583-2586): k=2 brute-force match of every
 * query descriptor against the match frame + Lowe ratio. desc are 32-byte ORB
 * descriptors. Output pairs (i_query, i_match) in query order; *k = count. */
int kmx_lcd_knn2(int norm, double lowe_ratio, const uint8_t* q, int32_t nq,
                 const uint8_t* mdesc, int32_t nm, int32_t* pairs_out,
                 int32_t* k);

/* Batched verification of candidates (verifyLoopSpin -> computeMatchedIndices
 * -> geometricVerificationNister -> recoverPose, drawio:2638-2657). */
typedef struct kmx_lcd_batch_desc {
  int32_t n_frames;       /* frames in the descriptor/feature pool           */
  int32_t max_feats;      /* features per frame (stride)                     */
  const int32_t* n_feats; /* [n_frames]                                       */
  const uint8_t* desc;    /* [n_frames][max_feats][32]                        */
  const double* bearings; /* [n_frames][max_feats][3] unit bearing vectors    */
  const double* points;   /* [n_frames][max_feats][3] stereo points (or NaN)  */
  int32_t n_cand;
  const int32_t* cand_query; /* [n_cand] frame ids */
  const int32_t* cand_match; /* [n_cand] frame ids */
} kmx_lcd_batch_desc;

typedef struct kmx_lcd_result {
  int32_t n_matches;      /* after kNN + Lowe                                 */
  int32_t mono_inliers;   /* 2D-2D RANSAC inliers                             */
  int32_t stereo_inliers; /* 3D-3D inliers                                    */
  int32_t accepted;       /* mono >= min_2d2d && (stereo >= min_3d3d, or
                             pnp >= min_2d3d with pose_recovery_type 1)     */
  int32_t iterations_2d2d;
  int32_t pnp_inliers;    /* 2D-3D inliers (pose_recovery_type 1)              */
  double T_query_match[12]; /* R row-major, t                                 */
} kmx_lcd_result;

typedef struct kmx_lcd kmx_lcd;
int kmx_lcd_create(const kmx_lcd_params* params, int device, kmx_lcd** out);
int kmx_lcd_destroy(kmx_lcd* h);
int kmx_lcd_set_stream(kmx_lcd* h, void* hip_stream);
/* Upload the frame pool (host arrays) to the device; kept until replaced.
 * Replaces every resident frame (a whole-pool reload); frames that arrive one
 * at a time go through kmx_lcd_add_frames. */
int kmx_lcd_set_frames(kmx_lcd* h, const kmx_lcd_batch_desc* pool);
/* LoopClosureDetector::addVLCFrame (drawio:2601; Kimera-Distributed adds each
 * VLC frame as it arrives, drawio:441-505): append n frames (max_feats must
 * equal the pool's, or set it on an empty handle). Resident frames are never
 * re-uploaded: the device pool grows by capacity doubling (one device-to-
 * device copy per doubling), the sampler table is kept (it depends only on
 * the parameters and max_feats). *first_id = id of the first appended frame. */
int kmx_lcd_add_frames(kmx_lcd* h, int32_t n, int32_t max_feats, const int32_t* n_feats,
                       const uint8_t* desc, const double* bearings, const double* points,
                       int32_t* first_id);
/* Frames resident (added or set) and the device capacity in frames. */
int kmx_lcd_pool_info(kmx_lcd* h, int32_t* n_frames, int32_t* capacity, int32_t* max_feats);
/* Verify n_cand candidates against the resident pool. results: n_cand records.
 * inlier masks (optional, may be NULL): [n_cand][max_feats] bytes, bit0 = 2D-2D
 * inlier, bit1 = 3D-3D inlier, indexed by match index (position in the pair
 * list of kmx_lcd_knn2 order). */
int kmx_lcd_verify(kmx_lcd* h, int32_t n_cand, const int32_t* cand_query,
                   const int32_t* cand_match, kmx_lcd_result* results,
                   uint8_t* inlier_masks);
/* Enqueue verification of candidates already resident on the device without
 * host synchronisation (benchmark / streaming path). Up to four calls are in
 * flight (candidate slots used in turn; a fifth waits for the first); calls
 * under 96 candidates per CU run their RANSACs concurrently. Results are not
 * returned: kmx_lcd_sync waits for every call (the synchronous entry points
 * return results). */
int kmx_lcd_verify_async(kmx_lcd* h, int32_t n_cand, const int32_t* cand_query,
                         const int32_t* cand_match);
int kmx_lcd_sync(kmx_lcd* h);
/* computeMatchedIndices (drawio:2583-2586) on resident frames, batched: for
 * candidate i the kNN2 + Lowe pairs of frames cand_query[i] / cand_match[i]
 * in query order, pairs_out[i][k] = (i_query, i_match) for k < k_out[i]
 * (pairs_out: [n_cand][max_feats][2]). */
int kmx_lcd_match(kmx_lcd* h, int32_t n_cand, const int32_t* cand_query, const int32_t* cand_match,
                  int32_t* pairs_out, int32_t* k_out);
/* geometricVerificationNister and / or recoverPose (drawio:2589-2598) on
 * caller-supplied correspondences, batched over candidates, no kNN2: the
 * pairs of candidate i are (i_query[k], i_match[k]) for k in
 * [mptr[i], mptr[i+1]) (feature indices of frames cand_query[i] /
 * cand_match[i]; at most max_feats pairs per candidate). stages: a mask of
 * KMX_LCD_STAGE_*.
 *   - without KMX_LCD_STAGE_2D2D every pair is a 2D-2D inlier (the
 *     correspondences are geometricVerificationNister's inliers) and, for the
 *     1-point 3D-3D recovery, the rotation is T_prior[i] (R row-major, t;
 *     [n][12]; required then, otherwise may be NULL);
 *   - without KMX_LCD_STAGE_RECOVER, accepted = mono_inliers >= min_2d2d and
 *     T_query_match = the 2D-2D pose (unit-norm t).
 * results / inlier_masks as kmx_lcd_verify, masks indexed by pair position. */
int kmx_lcd_verify_matches(kmx_lcd* h, int32_t n_cand, const int32_t* cand_query,
                           const int32_t* cand_match, const int64_t* mptr,
                           const int32_t* i_query, const int32_t* i_match, int stages,
                           const double* T_prior, kmx_lcd_result* results,
                           uint8_t* inlier_masks);
/* Instrumentation: when enabled, every verification brackets its kNN2 launch
 * and its RANSAC launches with HIP events; read_timing synchronises and
 * returns the device times (ms) of the last evented verification. */
int kmx_lcd_enable_timing(kmx_lcd* h, int enable);
int kmx_lcd_read_timing(kmx_lcd* h, double* knn_ms, double* ransac_ms);


/* ------------------------------------------------------------------------- */
/* Kimera-Multi-LCD BoW candidate stage: DBoW2 inverted-file L1 query         */
/* ------------------------------------------------------------------------- */
/* Replaces DBoW2 Database::queryL1 and L1Scoring::score as used by
 * LoopClosureDetector::detectLoop / detectLoopWithRobot (drawio:2574-2580,
 * 2612-2633; LcdParams.yaml:3-12). BowVectors are CSR: vptr[n+1] (int64),
 * words (uint32, strictly increasing per vector) and weights (L1-normalised
 * double). Entry id = position in the database.
 *
 * Weights. Every weight of a BowVector is finite and > 0 (DBoW2 stores no
 * other: `if (w > 0) addWeight`, then the L1 normalisation). The query reads
 * an accumulator of exactly 0.0 as "entry not touched yet", which holds because
 * every contribution |q - d| - |q| - |d| of such weights is negative. Database
 * vectors are checked on the host (kmx_bow_set_database, kmx_bow_add_entries:
 * KMX_EINVAL, the database unchanged); for query vectors passed as host arrays
 * the same rule is the caller's contract and is not checked.
 *
 * KMX_EUNSUP from a query. The best max_results entries are selected without
 * sorting the database: up to 6 histogram passes of 1024 bins narrow the range
 * [-2, 0] of the accumulator (cell widths 2^-9, 2^-19, ..., 2^-59) until the
 * entries certainly selected plus the cell holding the cut fit a sort buffer of
 * 2048 entries (KMX_BOW_LDS=0), or of 1024 entries per chunk of at most 14336
 * consecutive entry ids (the default; KMX_BOW_CHUNK sets a smaller chunk,
 * rounded up to a multiple of 16). The unsealed tail (<= 1024 entries) has room
 * of its own. Cells of width 2^-59 separate all distinct scores >= 0.5, so the
 * selection fails only when more entries than a buffer holds have (nearly)
 * identical scores and the cut falls among them: a tie group that lies wholly
 * behind the cut does not count. Then the call returns KMX_EUNSUP and its
 * outputs are unspecified; the database is unchanged and the handle stays
 * usable: the next call is answered as if the failed one had not been made. */
typedef struct kmx_bow kmx_bow;
int kmx_bow_create(int device, kmx_bow** out);
int kmx_bow_destroy(kmx_bow* h);
int kmx_bow_set_stream(kmx_bow* h, void* hip_stream);
/* Build the inverted file of entries 0..n_entries-1 (Database::add in order).
 * The vectors are checked on the host before any device call, the database
 * unchanged on failure: KMX_EINVAL as for kmx_bow_add_entries. */
int kmx_bow_set_database(kmx_bow* h, int32_t n_words, int32_t n_entries,
                         const int64_t* vptr, const uint32_t* words,
                         const double* weights);
/* queryL1 for nq query vectors: results with entry id < max_id[q] (NULL or
 * -1: all), sorted by score descending (ties: lower entry id first), at most
 * max_results (<= 256) each. out_n[nq]; out_ids / out_scores [nq][max_results];
 * score = 1 - 1/2 |v - w|_1. KMX_EUNSUP (above): too many tied scores at the cut
 * of some query for the sort buffer (2048 entries, or 1024 per chunk); the
 * outputs are unspecified and the handle stays usable. */
int kmx_bow_query(kmx_bow* h, int32_t nq, const int64_t* qptr,
                  const uint32_t* words, const double* weights,
                  const int32_t* max_id, int32_t max_results, int32_t* out_n,
                  int32_t* out_ids, double* out_scores);
/* Enqueue only (benchmark path); kmx_bow_sync waits, kmx_bow_fetch waits and
 * reports. */
int kmx_bow_query_async(kmx_bow* h, int32_t nq, const int64_t* qptr,
                        const uint32_t* words, const double* weights,
                        const int32_t* max_id, int32_t max_results);
int kmx_bow_sync(kmx_bow* h);
/* L1Scoring::score of n pairs (a_i, b_i) (the nss factor). */
int kmx_bow_score_pairs(kmx_bow* h, int32_t n, const int64_t* aptr,
                        const uint32_t* aw, const double* av,
                        const int64_t* bptr, const uint32_t* bw,
                        const double* bv, double* out);

/* ---- Streaming database: DBoW2 Database::add, one keyframe or batch at a
 * time. Every entry's vector stays resident on the device (a forward store);
 * entries [0, n_sealed) are in the inverted file, the tail [n_sealed,
 * n_entries) is scored per query from the forward store and merged in. After
 * any sequence of set_database / add calls every query returns bit for bit
 * what kmx_bow_set_database of the same vectors returns. Query vectors must be
 * BowVectors (words strictly increasing). kmx_bow_set_database keeps its
 * behaviour: it replaces everything and leaves all entries sealed. */
struct kmx_voc; /* below */
/* An empty database over n_words words (= set_database with 0 entries). Reads
 * KMX_BOW_LDS, KMX_BOW_CHUNK and KMX_BOW_TAIL, as kmx_bow_set_database does. */
int kmx_bow_reset(kmx_bow* h, int32_t n_words);
/* Database::add of n host vectors in order; the first gets id n_entries
 * (*first_id_out, may be NULL). Checked on the host before any device call,
 * the database unchanged on failure: KMX_EINVAL for a non-monotone vptr, words
 * not strictly increasing, a word >= n_words, a weight that is not finite and
 * > 0 (zero, -0.0, negative, NaN, infinite; a denormal is legal), null weights
 * with words present, or totals >= INT32_MAX; KMX_ESTATE without a database. An empty vector is a legal entry. */
int kmx_bow_add_entries(kmx_bow* h, int32_t n, const int64_t* vptr,
                        const uint32_t* words, const double* weights,
                        int32_t* first_id_out);
/* Append the vectors voc's last kmx_voc_transform*[_async] left on the device,
 * ordered after voc's stream; no word or weight passes through the host.
 * KMX_EINVAL when voc's word count differs from the database's; KMX_ESTATE
 * when voc holds no batch. The transform emits positive finite weights only. */
int kmx_bow_add_from_voc(kmx_bow* h, struct kmx_voc* voc, int32_t* first_id_out, int32_t* n_out);
/* Move the tail into the inverted file now (on the device). An add seals by
 * itself when the tail holds more than tail_cap entries. */
int kmx_bow_seal(kmx_bow* h);
/* tail_cap in [0, 1024] (the tail's sort capacity); default 64. The
 * environment variable KMX_BOW_TAIL, read at set_database / reset, overrides. */
int kmx_bow_set_tail_cap(kmx_bow* h, int32_t cap);
/* Any pointer may be NULL. device_bytes: inverted file, scratch and forward store. */
int kmx_bow_info(kmx_bow* h, int32_t* n_words, int32_t* n_entries, int32_t* n_sealed,
                 int32_t* tail_cap, int64_t* n_postings, int64_t* device_bytes);
/* Read stored vectors [first, first + n) back as CSR: vptr_out[n + 1] from 0.
 * words_out == NULL fills only vptr_out (to size the arrays); otherwise
 * words_out / weights_out hold `cap` >= vptr_out[n] elements. */
int kmx_bow_get_entries(kmx_bow* h, int32_t first, int32_t n, int64_t* vptr_out,
                        uint32_t* words_out, double* weights_out, int64_t cap);
/* kmx_bow_query with query q = stored entry entry_ids[q] of src (src may be h
 * or another database on the same device); ordered after src's stream; no
 * query words are uploaded. src's forward store must not grow while a query
 * that reads it is in flight. KMX_EUNSUP as for kmx_bow_query (buffers of 2048
 * entries, or 1024 per chunk); the handle stays usable. */
int kmx_bow_query_entries(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids,
                          const int32_t* max_id, int32_t max_results, int32_t* out_n,
                          int32_t* out_ids, double* out_scores);
int kmx_bow_query_entries_async(kmx_bow* h, kmx_bow* src, int32_t nq,
                                const int32_t* entry_ids, const int32_t* max_id,
                                int32_t max_results);
/* Wait for the last kmx_bow_query_async / kmx_bow_query_entries_async (same nq
 * and max_results) and copy its results out, as the synchronous forms do:
 * KMX_EUNSUP when that query's selection failed (buffers of 2048 entries, or
 * 1024 per chunk); the handle stays usable, and a later query and its fetch
 * are unaffected. */
int kmx_bow_fetch(kmx_bow* h, int32_t nq, int32_t max_results, int32_t* out_n,
                  int32_t* out_ids, double* out_scores);
/* L1Scoring::score of stored entries (a_ids[i], b_ids[i]) of src; an id of -1
 * (no entry) or an empty vector scores 0. */
int kmx_bow_score_entries(kmx_bow* src, int32_t n, const int32_t* a_ids,
                          const int32_t* b_ids, double* out);

/* ---- detectLoop / detectLoopWithRobot decided on the device: the nss gate,
 * the alpha cut, computeIslands and checkTemporalConstraint run on the query
 * results where kmx_bow_query_entries_async leaves them, and one record per
 * query comes back. The temporal constraint's state
 * {temporal_entries, latest_query_id, latest island start, latest island end}
 * lives in the handle and persists across calls, so any split of a keyframe
 * stream into calls gives the answers of one call. */
enum {
  KMX_BOW_NO_MATCHES = 0,
  KMX_BOW_LOW_NSS_FACTOR = 1,
  KMX_BOW_LOW_SCORE = 2,
  KMX_BOW_NO_GROUPS = 3,
  KMX_BOW_FAILED_TEMPORAL_CONSTRAINT = 4,
  KMX_BOW_LOOP_DETECTED = 5
};
enum {
  KMX_BOW_MODE_INTRA = 0, /* detectLoop: islands and the temporal constraint */
  KMX_BOW_MODE_INTER = 1  /* detectLoopWithRobot: the top result, no temporal stage */
};
/* LcdParams.yaml:3-12. Checked on the host before any device call (KMX_EINVAL):
 * use_nss 0 or 1, alpha and min_nss_factor finite, max_db_results in [1, 256],
 * the six integers below it >= 0. */
typedef struct {
  int32_t use_nss;
  double alpha;
  double min_nss_factor;
  int32_t max_db_results;
  int32_t recent_frames_window;
  int32_t max_intraisland_gap;
  int32_t min_matches_per_island;
  int32_t max_nrFrames_between_queries;
  int32_t max_nrFrames_between_islands;
  int32_t min_temporal_matches;
} kmx_bow_detect_params;
/* One per query (48 bytes). match_id is -1 and score 0.0 unless status is
 * FAILED_TEMPORAL_CONSTRAINT or LOOP_DETECTED; then they are the best island's
 * best member (inter mode: the top result). n_kept: results that passed the
 * alpha cut (0 when the query was settled before it). island_start / _end /
 * island_score: the best island (-1, -1, 0.0 without one). nss: the factor
 * the cut used (1.0 without use_nss); 0.0 when there is no previous keyframe. */
typedef struct {
  int32_t query_id;
  int32_t status;
  int32_t match_id;
  int32_t n_kept;
  int32_t island_start;
  int32_t island_end;
  double score;
  double nss;
  double island_score;
} kmx_bow_detect_record;
/* Query q = stored entry entry_ids[q] of src (NULL: h). One call enqueues on
 * h's stream, after src's: the gather and the query (intra: max_id =
 * max(id - recent_frames_window, 0); inter: none), the nss factor against
 * entry id - 1 of src, the decision, and in intra mode the temporal pass over
 * the queries in order; then one device-to-host copy and one synchronise.
 * Intra mode takes src == h (a robot queries its own database) and reports a
 * query of entry 0 as LOW_NSS_FACTOR when use_nss is set. records_out[nq];
 * cand_out (may be NULL) holds (query id, match id) of every LOOP_DETECTED in
 * query order, room for 2 * nq ints; *n_cand_out their count (intra mode; 0
 * in inter mode). KMX_EINVAL for bad params or an entry id outside src,
 * KMX_ESTATE without a database; the handle stays usable.
 * KMX_EUNSUP when the selection of some query of the call failed (as for
 * kmx_bow_query: buffers of 2048 entries, or 1024 per chunk): no record or
 * candidate is written, the temporal pass does not run, so the temporal state
 * is what it was before the call, and the handle stays usable. */
int kmx_bow_detect_entries(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids,
                           int32_t mode, const kmx_bow_detect_params* params,
                           kmx_bow_detect_record* records_out, int32_t* cand_out,
                           int32_t* n_cand_out);
int kmx_bow_detect_entries_async(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids,
                                 int32_t mode, const kmx_bow_detect_params* params);
/* Wait for the last kmx_bow_detect_entries_async (same nq) and copy out.
 * KMX_EUNSUP as for kmx_bow_detect_entries: nothing is written, the temporal
 * state is untouched by the failed call, the handle stays usable. */
int kmx_bow_detect_fetch(kmx_bow* h, int32_t nq, kmx_bow_detect_record* records_out,
                         int32_t* cand_out, int32_t* n_cand_out);
/* The same decision on caller-supplied query results: n[nq], ids / scores
 * [nq][K] sorted by score descending (ties: lower id first, ids unique per
 * query), K in [1, 256] (the row stride; params->max_db_results is not read
 * here), n[q] in [0, K], else KMX_EINVAL.
 * query_ids[nq] (NULL: 0 .. nq - 1) are the keyframe ids the temporal
 * constraint sees; nss[nq] and has_prev[nq] (either may be NULL: 1.0 / all 1)
 * the nss factors and whether a previous keyframe exists. use_state != 0: the
 * temporal pass starts from the handle's state and leaves it updated; 0: it
 * starts from zeros and the handle's state is untouched. No selection runs
 * here (the results are the caller's), so this call has no sort buffer to
 * overflow and never returns KMX_EUNSUP; a caller that got KMX_EUNSUP from a
 * query has no results to pass. */
int kmx_bow_decide_results(kmx_bow* h, int32_t nq, int32_t K, const int32_t* query_ids,
                           const int32_t* n, const int32_t* ids, const double* scores,
                           const double* nss, const int32_t* has_prev, int32_t mode,
                           const kmx_bow_detect_params* params, int32_t use_state,
                           kmx_bow_detect_record* records_out);
/* The temporal constraint's state, 4 x int32 (above). kmx_bow_reset and
 * kmx_bow_set_database zero it. */
int kmx_bow_get_temporal_state(kmx_bow* h, int32_t* state4_out);
int kmx_bow_set_temporal_state(kmx_bow* h, const int32_t* state4);
/* With timing on, a detection call records events on the handle's stream;
 * kmx_bow_read_detect_timing waits and returns the last call's milliseconds:
 * {gather + query + nss factor, k_bow_decide, k_bow_temporal}. */
int kmx_bow_enable_timing(kmx_bow* h, int on);
int kmx_bow_read_detect_timing(kmx_bow* h, double* ms3_out);

/* ------------------------------------------------------------------------- */
/* DBoW2 vocabulary transform: ORB descriptors -> BowVectors                  */
/* ------------------------------------------------------------------------- */
/* Replaces DBoW2 TemplatedVocabulary<FORB>::transform(features, BowVector&)
 * for the ORB vocabulary named at launch/kimera_vio_jackal.launch:40 [U: DBoW2
 * is not vendored; restated from the published algorithm, parity unpinned].
 * A descriptor (256 bits) descends from the root: among a node's children in
 * stored order it takes the one of least Hamming distance (the first of equal
 * children) until it reaches a node without children; that leaf's word id and
 * weight are its result. A frame's vector is, per weighting,
 *   TF_IDF / TF:   v[word] += weight, one addition per occurrence;
 *   IDF / BINARY:  v[word]  = weight;
 * over the features whose leaf weight is > 0, then divided by its L1 norm
 * (summed in increasing word id). The output is the CSR row kmx_bow_* reads:
 * words strictly increasing, weights double. */
#define KMX_VOC_TF_IDF 0
#define KMX_VOC_TF 1
#define KMX_VOC_IDF 2
#define KMX_VOC_BINARY 3

typedef struct kmx_voc kmx_voc;
/* The tree in DBoW2's node ids: node 0 is the root (parent[0] is not read), a
 * node's children are the nodes naming it as parent, in increasing node id
 * (DBoW2's load order). descriptor: n_nodes x 32 bytes; weight: per node (read
 * at leaves); word_node[w]: the leaf of word w. Checked before any device
 * call: KMX_EINVAL for n_nodes < 2, a parent out of range, a cycle or a depth
 * over 64, a word that maps to an inner node, a leaf that is no word or two
 * words; KMX_EUNSUP for an unknown weighting. */
int kmx_voc_create(int device, int32_t n_nodes, const int32_t* parent,
                   const uint8_t* descriptor, const double* weight, int32_t n_words,
                   const int32_t* word_node, int weighting, kmx_voc** out);
int kmx_voc_destroy(kmx_voc* h);
int kmx_voc_set_stream(kmx_voc* h, void* hip_stream);
/* Shape of the resident tree (any pointer may be NULL): the largest child
 * count, the deepest leaf, the nodes of the tree's top kept in LDS, and the
 * workgroups of the descent kernel (those resident at once on the device). */
int kmx_voc_info(kmx_voc* h, int32_t* n_nodes, int32_t* n_words, int32_t* max_children,
                 int32_t* max_depth, int32_t* lds_nodes, int32_t* descend_grid);
/* Transform n_frames frames of host descriptors desc[n_frames][max_feats][32]
 * (1 <= max_feats <= 1024; frame f has n_feats[f] features; bytes beyond them
 * are never read into the result). out_nnz[n_frames]; frame f's vector is
 * out_words / out_weights [f * max_feats .. f * max_feats + out_nnz[f]). */
int kmx_voc_transform(kmx_voc* h, int32_t n_frames, int32_t max_feats, const int32_t* n_feats,
                      const uint8_t* desc, int32_t* out_nnz, uint32_t* out_words,
                      double* out_weights);
/* The same on frames resident in a detector's device pool (kmx_lcd_set_frames
 * / kmx_lcd_add_frames): nothing is uploaded again. frame_ids[n] may repeat
 * and come in any order; the stride of the outputs is the pool's max_feats.
 * Ordered after the work enqueued on the detector's stream. KMX_EINVAL for an
 * id outside the pool or a pool on another device. */
int kmx_voc_transform_pool(kmx_voc* h, kmx_lcd* pool, int32_t n, const int32_t* frame_ids,
                           int32_t* out_nnz, uint32_t* out_words, double* out_weights);
/* Enqueue only (benchmark path); kmx_voc_sync waits. The results stay on the
 * device. A pool transform in flight reads the pool's buffers: wait for it
 * before the pool grows or is replaced. */
int kmx_voc_transform_async(kmx_voc* h, int32_t n_frames, int32_t max_feats,
                            const int32_t* n_feats, const uint8_t* desc);
int kmx_voc_transform_pool_async(kmx_voc* h, kmx_lcd* pool, int32_t n, const int32_t* frame_ids);
int kmx_voc_sync(kmx_voc* h);
/* Instrumentation: when enabled, every transform brackets its descent and its
 * per-frame reduction with HIP events; read_timing synchronises and returns
 * the device times (ms) of the last transform. */
int kmx_voc_enable_timing(kmx_voc* h, int enable);
int kmx_voc_read_timing(kmx_voc* h, double* descend_ms, double* reduce_ms);

/* ------------------------------------------------------------------------- */
/* Chordal initialisation of a batch of pose graphs (dpgo's local
 * initialisation method Chordal [U: dpgo is not vendored; restated from the
 * SE-Sync chordal relaxation]; the problem kmx.dpgo.init.chordal_initialization
 * solves on the host). Additive to ABI 10, like kmx_pgo_get_tcg_groups.
 * Poses 0..n-1 are cut into n_blocks contiguous blocks (a robot each; one block
 * over everything is a centralised solve). An edge (i, j, R_ij, t_ij, kappa,
 * tau, w) means R_j = R_i R_ij, t_j = t_i + R_i t_ij; both ends lie in one
 * block. Anchors are held at R = I, t = 0.
 *   1. minimise sum w kappa |X_j - X_i R_ij|_F^2 over unconstrained 3x3 blocks;
 *   2. project every free block to SO(3) (SVD, determinant fix on the smallest
 *      singular direction);
 *   3. minimise sum w tau |t_j - t_i - R_i t_ij|^2 with those rotations.
 * Steps 1 and 3 are Jacobi-preconditioned conjugate gradients, one per block
 * and per right-hand side (the three rows of X, the three components of t):
 * the stop test |r| <= rtol |b| and the iteration count are per (block, row),
 * so a block's result does not depend on the other blocks of the batch. Two
 * solves of the same graph give the same bits, whatever check_every is. */
typedef struct kmx_chordal kmx_chordal;
typedef struct {
  double rtol;            /* 0: 1e-10 */
  int32_t max_iterations; /* per stage; 0: 20000 */
  int32_t check_every;    /* iterations enqueued between two host reads of the
                             device's done word; 0: 50. No effect on the result. */
} kmx_chordal_params;
typedef struct {          /* per block */
  int32_t iterations_rot, iterations_trans; /* the largest count among the block's three CGs */
  int32_t converged;      /* 1: all six met the stop test; 0: max_iterations cut one short */
  double relres_rot[3], relres_trans[3]; /* |r| / |b| at the end (0 where |b| = 0) */
} kmx_chordal_block_info;
int kmx_chordal_create(int device, kmx_chordal** out);
int kmx_chordal_destroy(kmx_chordal* h);
int kmx_chordal_set_stream(kmx_chordal* h, void* hip_stream);
/* Checked on the host before any device call; on failure the handle keeps its
 * previous graph: KMX_EINVAL for an index out of range, src == dst, an edge
 * across blocks, a value that is not finite, kappa or tau <= 0, w < 0, a
 * block_ptr that is not monotone from 0 to n_poses, an anchor out of range or
 * listed twice, and a connected component over the edges of w > 0 without an
 * anchor (a free pose without such an edge is one): that system is singular.
 * Edges of w == 0 contribute nothing. Parallel edges and empty blocks are
 * legal. R is [n_edges][9] row-major, t [n_edges][3]; weight NULL: 1. */
int kmx_chordal_set_graph(kmx_chordal* h, int32_t n_poses, int32_t n_blocks, const int32_t* block_ptr,
                          int64_t n_edges, const int32_t* src, const int32_t* dst,
                          const double* R, const double* t,
                          const double* kappa, const double* tau, const double* weight,
                          int32_t n_anchors, const int32_t* anchors);
/* New weights for the same edges ([n_edges]; NULL: 1): only the weights are
 * uploaded again. Checked like set_graph's; on KMX_EINVAL the previous weights
 * stay in force. */
int kmx_chordal_set_weights(kmx_chordal* h, const double* weight);
/* R_init [n][9] / t_init [n][3]: the start vectors (NULL: zero; values at
 * anchors are ignored). R_out [n][9], t_out [n][3]; info [n_blocks] or NULL.
 * p NULL or a field 0: the default. Reaching max_iterations is no error: that
 * block reports converged = 0 and the output is its last iterate, projected.
 * A (block, row) whose right-hand side is zero is converged at once and keeps
 * its start vector. KMX_ESTATE without a graph. */
int kmx_chordal_solve(kmx_chordal* h, const kmx_chordal_params* p,
                      const double* R_init, const double* t_init,
                      double* R_out, double* t_out, kmx_chordal_block_info* info);
/* Device times (ms, HIP events) of the last solve: the upload of the start
 * vectors, the rotation stage with the projection, the translation stage, the
 * download. KMX_ESTATE before the first solve. */
int kmx_chordal_get_timing(kmx_chordal* h, double* ms /* [4] */);

/* Robust chordal initialisation: GNC-TLS around the two solves, decided on the
 * device (dpgo's robust local initialisation [U: dpgo is not vendored; the rule
 * is kmx.dpgo.init.robust_chordal_initialization's, restated from the published
 * GNC algorithm, Yang et al. 2020]). With
 *   r^2 = kappa |R_j - R_i R_ij|_F^2 + tau |t_j - t_i - R_i t_ij|^2
 * (dpgo's computeMeasurementError [U]; kappa and tau unscaled, on the projected
 * rotations) and c = barc, an edge's factor for a block's mu is
 *   g = 1 for r^2 <= mu/(mu+1) c^2, g = 0 for r^2 >= (mu+1)/mu c^2,
 *   g = sqrt(c^2 mu (mu+1) / r^2) - mu in between,
 * fixed edges keep g = 1, and the edge's weight in a solve is w0 g (w0: the
 * handle's weight from set_graph / set_weights; an edge of w0 = 0 stays out and
 * is not counted). The first solve runs at g = 1. From its residuals a block
 * takes mu_0 (mu_init, or c^2 / (2 max r^2 - c^2) over its counted edges; with
 * 2 max r^2 <= c^2 it is done with 0 updates). Then, per block: g from the last
 * solve's residuals and mu; done (converged) when every g is 0 or 1 and none
 * differs from the g of the last solve; otherwise one more solve with w0 g,
 * warm-started (an update), and mu <- mu mu_step. A block stops after
 * max_updates updates with converged = 0. mu, the counts and the done flag are
 * per block and live on the device; a done block is frozen (no CG, no
 * projection, no weight is rewritten), so a block's result does not depend on
 * the other blocks of the batch, bit for bit. */
typedef struct {
  double barc;         /* 0: 5.0 (kmx_pgo's GNCBarc default) */
  double mu_init;      /* 0: per block from its largest residual, c^2 / (2 max r^2 - c^2); > 0: fixed (dpgo: 1e-5) */
  double mu_step;      /* 0: 1.4 */
  int32_t max_updates; /* 0: 100 */
  int32_t reserved;    /* 0. (1: every update's rotation CG starts from the projected rotations and not
                          from the previous unprojected iterate; kept for the measurement of DESIGN.md 14) */
} kmx_chordal_robust_params;
typedef struct {       /* per block */
  int32_t updates;     /* solves after the first */
  int32_t converged;   /* 0: max_updates cut it short */
  int32_t n_kept, n_rejected, n_fractional; /* the returned g over the edges that are not fixed and have w0 > 0 */
  int32_t reserved;
  double mu;           /* the mu the returned g was formed with (0: no g was formed) */
} kmx_chordal_robust_info;

/* dpgo's computeMeasurementError [U] on caller-supplied poses (R [n][9],
 * t [n][3], used as given, anchors included), and, with mu != NULL, the GNC-TLS
 * factor of every edge for mu[block]: the loop's own kernel. Edges of w0 = 0
 * are evaluated like any other; fixed edges report g = 1. The handle's
 * weights and graph are untouched. KMX_ESTATE without a graph. */
int kmx_chordal_residuals(kmx_chordal* h, const double* R, const double* t,
                          const double* mu /* [n_blocks] or NULL */, double barc /* 0: 5.0 */,
                          const uint8_t* fixed /* [n_edges] or NULL: none */,
                          double* r2_out /* [n_edges] */, double* g_out /* [n_edges] or NULL */);
/* The loop above. p as in kmx_chordal_solve (every solve of the loop), rp NULL
 * or a field 0: the default. Checked on the host before any device call, the
 * handle untouched on failure: the parameters finite and >= 0, mu_step > 1
 * when given; and the fixed edges of w0 > 0 must BY THEMSELVES connect every
 * free pose to an anchor (fixed NULL: no edge is fixed), KMX_EINVAL otherwise.
 * That precondition is what lets the device choose the other weights, down to
 * 0, without a connectivity check on the host per update: whatever it chooses,
 * both systems stay positive definite. g_out [n_edges] (or NULL): the factors
 * of the last solve; info [n_blocks] (or NULL): a block's last solve;
 * rinfo [n_blocks] (or NULL). The handle's weights are not changed: a
 * kmx_chordal_solve after it gives the bits it gave before. */
int kmx_chordal_solve_robust(kmx_chordal* h, const kmx_chordal_params* p,
                             const kmx_chordal_robust_params* rp, const uint8_t* fixed,
                             const double* R_init, const double* t_init, double* R_out, double* t_out,
                             double* g_out, kmx_chordal_block_info* info /* last update's solve */,
                             kmx_chordal_robust_info* rinfo);
/* Figures of the last kmx_chordal_solve_robust (HIP events and device-side
 * counts): [0] device ms of the whole call, [1] of the first (cold) solve,
 * [2] of all GNC passes and decisions together, [3] their number, [4] / [5] CG
 * iterations of the rotation / translation stage summed over the blocks and
 * solves (a block's largest row count per solve), [6] solves run by the host
 * loop (the first included), [7] 0. KMX_ESTATE before the first robust solve. */
int kmx_chordal_get_robust_stats(kmx_chordal* h, double* out /* [8] */);

/* ------------------------------------------------------------------------- */
/* Dual optimality certificate of an RBCD solution (DESIGN.md
 * 16): the smallest eigenvalue of S(X) = Q - Lambda(X) by Lanczos on the
 * device. Additive to ABI 10. The graph is the TEAM graph on one device, poses
 * flattened to 0..n-1 (no blocks: S couples robots). An edge i -> j with
 * (R, t, kappa, tau, w) contributes, in 4x4 blocks ([rotation | translation]),
 *   Q_ii += w [[kappa I + tau t t^T, tau t], [tau t^T, tau]]
 *   Q_jj += w diag(kappa, kappa, kappa, tau)
 *   Q_ij -= w [[kappa R, tau t], [0^T, tau]],   Q_ji = Q_ij^T,
 * and Lambda_i = sym(Y_i^T (X Q)_{i,Y}) (3x3 per pose, zero on the translation
 * entry). X is [n][r][4], the layout of kmx_pgo_get_iterate with the robots
 * concatenated. X S is half the Riemannian gradient, so |X S|_F measures
 * stationarity, and X is the global optimum of the rank-r relaxation (and its
 * rounding the optimal trajectory) when S is positive semidefinite.
 * Sums are ordered (a pose's records in edge order, a fixed tree per tile of
 * 64 poses, one wave over the tile partials): two calls give the same bits. */
typedef struct kmx_cert kmx_cert;
#define KMX_CERT_UNDECIDED 0 /* max_steps reached (a result, not an error)          */
#define KMX_CERT_CERTIFIED 1 /* rho <= eta / 10 and theta_min - rho >= -eta: an
                                eigenvalue lies within rho of theta_min, the smallest
                                the Krylov space shows (no bound of lambda_min)      */
#define KMX_CERT_NEGATIVE 2  /* theta_min < -eta: S has an eigenvalue below -eta     */
typedef struct {
  double eta;          /* > 0, required: the tolerance of the decision              */
  int32_t max_steps;   /* 0: 5000                                                   */
  int32_t test_every;  /* the rule is applied at step counts that are multiples of
                          it; 0: 10                                                 */
  int32_t check_every; /* steps enqueued between two host reads; 0: 50. No effect
                          on the result.                                            */
  int32_t reserved;    /* 0 */
  uint64_t seed;       /* of the start vector                                       */
} kmx_cert_params;
typedef struct {
  int32_t decision;    /* KMX_CERT_*                                                */
  int32_t steps;       /* Lanczos steps the decision was taken on                   */
  double theta_min, theta_max; /* extreme Ritz values                              */
  double residual;     /* rho = |beta_k s_k|: |S y - theta_min y| for the Ritz vector y */
} kmx_cert_result;
typedef struct {
  double cost;          /* tr(X Q X^T) (twice kmx_pgo's cost)                       */
  double trace_lambda;  /* tr Lambda (= cost at a stationary point)                 */
  double stationarity;  /* |X S|_F                                                  */
} kmx_cert_point_info;
int kmx_cert_create(int device, kmx_cert** out);
int kmx_cert_destroy(kmx_cert* h);
int kmx_cert_set_stream(kmx_cert* h, void* hip_stream);
/* Checked on the host before any device call; on failure the handle keeps its
 * previous graph: KMX_EINVAL for an index out of range, src == dst, a value
 * that is not finite, kappa or tau <= 0, w < 0. Edges of w == 0 contribute
 * nothing; parallel edges, poses without edges (a zero row of S) and
 * n_edges == 0 are legal. R is [n_edges][9] row-major, t [n_edges][3]; weight
 * NULL: 1. A point set before is dropped. */
int kmx_cert_set_graph(kmx_cert* h, int32_t n_poses, int64_t n_edges, const int32_t* src, const int32_t* dst,
                       const double* R, const double* t, const double* kappa, const double* tau,
                       const double* weight);
/* New weights for the same edges ([n_edges]; NULL: 1); on KMX_EINVAL the
 * previous weights stay. A point that is set is evaluated again for them. */
int kmx_cert_set_weights(kmx_cert* h, const double* weight);
/* The point X [n][r][4]: forms the symmetric 4x4 D_i - Lambda_i of every pose
 * on the device. KMX_EINVAL for r outside 3..8 or a value that is not finite,
 * KMX_ESTATE without a graph; these leave the handle as it was. A HIP failure
 * (KMX_EHIP) after the upload has begun drops the point that was set: the
 * device's copy is being overwritten. info_out may be NULL. */
int kmx_cert_set_point(kmx_cert* h, int32_t r, const double* X, kmx_cert_point_info* info_out);
/* The loop's own kernels on caller data: Lambda_i (row-major 3x3) and
 * out = S v. KMX_ESTATE without a point. */
int kmx_cert_get_lambda(kmx_cert* h, double* out /* [n][9] */);
int kmx_cert_apply(kmx_cert* h, const double* v_in /* [4n] */, double* out /* [4n] */);
/* Plain Lanczos on S from the start vector of `seed` (no reorthogonalisation;
 * the basis is not stored), decided on the host from the coefficients at step
 * counts that are multiples of test_every; a breakdown (beta at the rounding
 * level of the tridiagonal) ends it with the rule applied to that prefix.
 * y_out != NULL: a second pass repeats the steps and accumulates the Ritz
 * vector of theta_min, normalised. KMX_ESTATE without a point. */
int kmx_cert_min_eig(kmx_cert* h, const kmx_cert_params* p, kmx_cert_result* res, double* y_out /* [4n] or NULL */);
/* alpha_j, beta_j of the last kmx_cert_min_eig, the steps the host has read
 * (*count_out of them; at most `capacity` are written). */
int kmx_cert_get_coefficients(kmx_cert* h, int32_t capacity, double* alpha_out, double* beta_out,
                              int32_t* count_out);
/* Host only: the decision rule on a caller's tridiagonal (alpha [k], beta [k];
 * beta[k-1] is the norm left after step k). KMX_EINVAL for eta <= 0 or k < 1. */
int kmx_cert_ritz(int32_t k, const double* alpha, const double* beta, double eta, kmx_cert_result* res);
/* Host only: the start vector of `seed` before its normalisation:
 * z = seed + (i+1) 0x9E3779B97F4A7C15, the splitmix64 finaliser, and
 * u_i = (z >> 11) 2^-52 - 1. */
int kmx_cert_start_vector(uint64_t seed, int64_t count, double* out);
/* Device times (ms, HIP events): [0] the last set_point's kernels; of the last
 * kmx_cert_min_eig (0 before one): [1] the Lanczos steps, an event pair around
 * each batch's launches with the spans summed, so the time the stream idles
 * while the host decides is not in it; [2] the vector pass's launches (0 without
 * y_out); [3] the transfers: both uploads of the start vector, every batch's
 * read-back of alpha and beta, the upload of s and the download of y.
 * KMX_ESTATE before the first set_point. */
int kmx_cert_get_timing(kmx_cert* h, double* ms /* [4] */);
/* Host times (ms, the host clock) of the last kmx_cert_min_eig: [0] the
 * decisions (the tridiagonal solver and the rule over all tests), [1] the
 * whole call, with enqueueing and the waits for the stream. */
int kmx_cert_get_host_timing(kmx_cert* h, double* ms /* [2] */);
/* The escape step of the Riemannian staircase, for a point of
 * rank r that kmx_cert_min_eig found NEGATIVE with the Ritz vector y. For each
 * alpha[k] the rank-(r+1) candidate [X; alpha[k] y^T] is formed on the device:
 * every pose's three rotation columns (length r + 1) are re-orthonormalised by
 * Gram-Schmidt in column order, applied twice (a positive diagonal: the QR
 * factor), the translation column passes through, and a pose whose new
 * rotation entries are all zero is copied as it is (alpha = 0 gives [X; 0]
 * exactly). cost_out[k] = tr(X+ Q X+^T) over the graph with the handle's
 * current weights, in the ordered sums of kmx_cert_set_point, so one call of 8
 * and 8 calls of 1 give the same bits. *best_out: the candidate of the lowest
 * finite cost strictly below the point's own cost (kmx_cert_set_point's, kept
 * in the handle), ties to the earlier index; -1 when no candidate descends (a
 * result, not an error). KMX_ESTATE without a point; KMX_EINVAL for n_alpha
 * outside 1..8 or an alpha or y that is not finite; KMX_EUNSUP for r == 8
 * (there is no rank 9). These leave the handle as it was. The handle owns the
 * candidates (n_alpha n (r+1) 32 bytes, grown on demand). */
int kmx_cert_escape(kmx_cert* h, const double* y /* [4n] */, int32_t n_alpha, const double* alpha /* [n_alpha] */,
                    double* cost_out /* [n_alpha] */, int32_t* best_out);
/* Downloads candidate k of the last kmx_cert_escape and makes it the handle's
 * point at rank r + 1 (kmx_cert_set_point's kernel on the device's copy; no
 * upload); info_out as kmx_cert_set_point fills it (or NULL). KMX_ESTATE
 * without a preceding kmx_cert_escape, or when kmx_cert_set_point,
 * kmx_cert_set_graph, kmx_cert_set_weights or a commit came after it;
 * KMX_EINVAL for k outside that call's candidates. */
int kmx_cert_escape_commit(kmx_cert* h, int32_t k, double* X_out /* [n][r+1][4] */,
                           kmx_cert_point_info* info_out);
/* Device times (ms, HIP events) of the last kmx_cert_escape (0 before one):
 * [0] its kernels (lift, cost, the reduction), [1] its transfers (the upload
 * of y and alpha, the download of the costs). */
int kmx_cert_get_escape_timing(kmx_cert* h, double* ms /* [2] */);

/* ------------------------------------------------------------------------- */
/* Mesh deformation (Kimera-PGMO's mesh update: embedded deformation,          */
/* Sumner et al. 2007, interpolation only)                                     */
/* ------------------------------------------------------------------------- */
/* [U: Kimera-PGMO is not vendored; restated from the published formulas.]
 * Additive to ABI 10. A streaming handle: control nodes and mesh vertices are
 * append-only.
 *
 * Control node j: a robot id, a stamp (ns), a rest pose (Rrest_j, g_j) and a
 * current pose (Rcur_j, p_j). Its correction is the rigid map
 *   A_j(x) = R_j (x - g_j) + p_j,  R_j = Rcur_j Rrest_j^T.
 * A node that was never given a current pose has current = rest. Within a
 * robot, node stamps are non-decreasing across appends.
 *
 * Vertex i: a robot id, a stamp s_i and a position v_i (fp32 in and out; all
 * arithmetic is fp64). Binding: the candidates are the nodes of the vertex's
 * robot with |s_j - s_i| <= window_ns (both ends inclusive, s_i -+ window_ns
 * saturating at the int64 limits), ranked by the squared distance
 *   d^2 = dx dx + dy dy + dz dz,  dx = double(v.x) - g.x, ...
 * (summed in that order, no contraction), ties to the lower node id. With m
 * candidates the vertex uses the min(m, k + 1) - 1 nearest and d_max is the
 * distance of the next one; m == 1 uses that node at weight 1; m == 0 leaves
 * the vertex unbound. Weights: w_j = (1 - d_j / d_max)^2 divided by their sum
 * (taken in rank order); when that sum is not > 0 (d_max == 0, or every used
 * node at d_max) the nearest node alone is used, at weight 1.
 * Deformation: v_i' = sum_j w_j A_j(v_i) in rank order, rounded to fp32 once;
 * an unbound vertex is returned as it is. Nodes appended after a vertex was
 * bound do not affect it until it is bound again. */
typedef struct kmx_mesh kmx_mesh;
typedef struct {
  int32_t k;         /* nodes per vertex, 1..8 (KMX_EUNSUP otherwise) */
  int32_t n_robots;  /* robot ids are 0..n_robots-1 */
  int64_t window_ns; /* W >= 0 */
} kmx_mesh_params;
typedef struct {
  int64_t n_nodes, n_vertices;
  int64_t node_capacity, vertex_capacity; /* device rows allocated */
  int64_t device_bytes;
  int32_t k, lds_nodes;           /* lds_nodes: the most node positions one workgroup of the bind kernel stages */
  int32_t last_bind_blocks;       /* workgroups of the last kmx_mesh_bind ... */
  int32_t last_bind_global_blocks; /* ... and those of them that read node positions from global memory */
} kmx_mesh_info_t;
typedef struct {
  int64_t n_vertices; /* of the call */
  int64_t n_unbound;  /* no candidate node: returned unmoved */
  int64_t n_partial;  /* bound to 1..k-1 nodes */
  double max_displacement;  /* max |v' - v| over the call's vertices, from the fp32 result */
  double sum_sq_displacement;
} kmx_mesh_stats;

int kmx_mesh_create(const kmx_mesh_params* params, int device, kmx_mesh** out);
int kmx_mesh_destroy(kmx_mesh* h);
int kmx_mesh_set_stream(kmx_mesh* h, void* hip_stream);
/* per_robot_nodes / per_robot_vertices: [n_robots], either may be NULL. */
int kmx_mesh_info(kmx_mesh* h, kmx_mesh_info_t* info, int64_t* per_robot_nodes, int64_t* per_robot_vertices);
/* Appends n nodes (ids n_nodes ..): robot[n], stamp_ns[n], Rrest[n][3][3] row
 * major, g[n][3]. KMX_EINVAL for a null array, a robot id out of range, a value
 * that is not finite or a stamp below its robot's newest; nothing is added then. */
int kmx_mesh_add_nodes(kmx_mesh* h, int64_t n, const int32_t* robot, const int64_t* stamp_ns,
                       const double* Rrest, const double* g);
/* Current poses of nodes [first, first + n): Rcur[n][3][3], p[n][3]; R_j is
 * formed on the device. KMX_EINVAL for a range outside the nodes or a value
 * that is not finite (nothing is changed). */
int kmx_mesh_set_node_poses(kmx_mesh* h, int64_t first, int64_t n, const double* Rcur, const double* p);
/* Appends n vertices, unbound; *first_id_out (or NULL) gets the first one's id. */
int kmx_mesh_add_vertices(kmx_mesh* h, int64_t n, const int32_t* robot, const int64_t* stamp_ns,
                          const float* xyz, int64_t* first_id_out);
/* Binds vertices [first, first + n) to the nodes present now. */
int kmx_mesh_bind(kmx_mesh* h, int64_t first, int64_t n);
/* idx[n][k] (node ids in rank order, -1 beyond count), w[n][k] (0 beyond
 * count), count[n]; any of the three may be NULL. */
int kmx_mesh_get_bindings(kmx_mesh* h, int64_t first, int64_t n, int32_t* idx, double* w, int32_t* count);
/* Deforms vertices [first, first + n) into xyz_out[n][3] (host) and waits.
 * stats_out (or NULL): reduced in a fixed order (workgroup partials, then one
 * wave), so identical from run to run. */
int kmx_mesh_deform(kmx_mesh* h, int64_t first, int64_t n, float* xyz_out, kmx_mesh_stats* stats_out);
/* The same into device memory dev_xyz_out[n][3] (fp32) on the handle's
 * stream; enqueues only, kmx_mesh_sync waits. */
int kmx_mesh_deform_device(kmx_mesh* h, int64_t first, int64_t n, void* dev_xyz_out);
int kmx_mesh_sync(kmx_mesh* h);
/* With timing on, bind and deform bracket their kernels with HIP events;
 * read_timing waits and returns the last bind's and the last deform's device
 * time in ms (0 for one that has not run since timing was enabled). */
int kmx_mesh_enable_timing(kmx_mesh* h, int enable);
int kmx_mesh_read_timing(kmx_mesh* h, double* bind_ms, double* deform_ms);

/* ------------------------------------------------------------------------- */
/* Deformation graph optimisation (Kimera-PGMO's solve over simplified mesh    */
/* vertices with keyframe priors; embedded deformation, Sumner et al. 2007):   */
/* Levenberg-Marquardt with block-Jacobi preconditioned CG                      */
/* ------------------------------------------------------------------------- */
/* [U: Kimera-PGMO is not vendored; restated from the published formulas.]
 * Additive to ABI 10. tests/dgraph_ref.py restates this text in numpy.
 *
 * Nodes and unknowns.
 *  - Nodes are 0..n-1, each with a rest pose (Rrest_i, g_i).
 *  - A keyframe's rest pose is its odometry pose. A control vertex has
 *    Rrest = I.
 *  - The unknown is (R_i, t_i), starting at the rest pose unless the caller
 *    sets a start.
 *
 * Deformation edges.
 *  - An edge is directed, e = (i -> j, w_e), with w_e finite and >= 0. A
 *    weight of 0 is kept and skipped.
 *  - A mesh edge or a keyframe-vertex link is two directed edges.
 *  - Formed once on the device when the graph is set:
 *    d_e = Rrest_i^T (g_j - g_i), each entry summed over the inner index in
 *    order.
 *  - Residual: r_e = R_i d_e + t_i - t_j. It is zero at rest.
 *  - Term: w_e |r_e|^2.
 *
 * Priors per node. mode_i in {0 none, 1 soft, 2 hard}.
 *  - Soft adds kappa_i |R_i - Rhat_i|_F^2 + tau_i |t_i - that_i|^2. kappa_i
 *    and tau_i are finite and >= 0.
 *  - Hard puts the node at (Rhat_i, that_i) and removes it from the unknowns.
 *    Its step is 0, and its edges still act on its neighbours.
 *
 * Well-posedness, checked on the host.
 *  - Run a union-find over the edges of weight > 0.
 *  - Every component must hold a hard node or a soft node with tau > 0.
 *  - Otherwise return KMX_EINVAL, and the handle stays as it was.
 *  - A free node whose rotation is not determined (fewer than two non-parallel
 *    outgoing edges and no kappa) is legal: the damping below keeps it where
 *    it is.
 *
 * Local update.
 *  - R_i <- Exp(omega_i) R_i (left, world frame) and t_i <- t_i + delta_i.
 *    That is 6 numbers per free node, in the order (omega, delta).
 *  - With a_e = R_i d_e the edge's linearisation is
 *    omega_i x a_e + delta_i - delta_j.
 *  - So an incidence record needs only `other`, `w` and `a_e`: 36 B, re-formed
 *    once per outer iteration.
 *  - The rotation prior's Gauss-Newton block is 2 kappa_i I.
 *
 * Levenberg-Marquardt. Cost f = the sum of the terms above; b = J^T r. The
 * first rules below follow GTSAM's LM with lambda I damping [U].
 *  - Each outer iteration solves (J^T J + lambda I) delta = -b and forms the
 *    trial point and its cost f+.
 *  - Accept iff f+ < f. A NaN f+ is a reject.
 *  - On accept: lambda <- max(lambda / factor, lambda_min). On reject:
 *    lambda <- lambda factor.
 *  - Stop reasons:
 *    1. an accepted step with f - f+ <= rel_tol f;
 *    2. f+ <= abs_tol (tested on an accepted step, before reason 1);
 *    3. max_iterations;
 *    4. lambda > lambda_max (tested after a reject);
 *    5. |b| = 0 at the start.
 *  - Defaults: lambda_init 1e-5, factor 10, lambda_min 1e-10, lambda_max 1e5,
 *    rel_tol 1e-5, abs_tol 0, max_iterations 100.
 *
 * Inner solve.
 *  - Conjugate gradients from delta = 0, the plain two-reduction form.
 *  - Preconditioned by the inverse of each free node's 6x6 diagonal block of
 *    J^T J + lambda I.
 *  - Stops at |r|_2 <= cg_rtol |b|_2 or cg_max_iterations. Defaults are 1e-6
 *    and 500.
 *
 * Sums are ordered (a node adds its records in edge order, a tile of 64 nodes
 * reduces by a fixed tree, one wave sums the tiles), so a solve is identical
 * from run to run and does not depend on check_every. */
typedef struct kmx_dgraph kmx_dgraph;
typedef struct {
  /* 0 (or, for abs_tol and rel_tol, a negative value) in a field: its default */
  double lambda_init, lambda_factor, lambda_min, lambda_max;
  double rel_tol;  /* < 0: the default; 0 is 0 */
  double abs_tol;  /* default 0 */
  double cg_rtol;
  int32_t max_iterations, cg_max_iterations;
  int32_t check_every; /* CG iterations enqueued between two reads of the stop word, default 50 */
  int32_t reserved;
} kmx_dgraph_params;
typedef struct {
  double cost_initial, cost_final, lambda_final, gradnorm_initial;
  int32_t iterations;    /* outer iterations run (accepted and rejected) */
  int32_t accepted;      /* of them accepted */
  int32_t stop_reason;   /* 1..5 above */
  int32_t cg_iterations; /* summed over the outer iterations */
} kmx_dgraph_result;
typedef struct {
  double cost, trial_cost, lambda;
  int32_t cg_iterations, accepted;
} kmx_dgraph_log_entry;
enum {
  KMX_DGRAPH_EVAL_COST = 0,   /* out[1] */
  KMX_DGRAPH_EVAL_GRAD = 1,   /* out[n][6]: b = J^T r, 0 at hard nodes */
  KMX_DGRAPH_EVAL_JTJ = 2,    /* out[n][6] = J^T J v for v[n][6]; hard nodes' rows of v are not read */
  KMX_DGRAPH_EVAL_BLOCKS = 3  /* out[n][21]: the upper triangles of the 6x6 diagonal blocks of J^T J, row by row */
};

int kmx_dgraph_create(int device, kmx_dgraph** out);
int kmx_dgraph_destroy(kmx_dgraph* h);
int kmx_dgraph_set_stream(kmx_dgraph* h, void* hip_stream);
/* Rrest[n][3][3] row major, g[n][3]; m directed edges src -> dst with weights
 * w[m] (NULL: all 1). KMX_EINVAL for a null array, n < 0, m < 0, an endpoint
 * out of range, a self-loop, a value that is not finite or a negative weight.
 * Poses go to rest and the priors are cleared. */
int kmx_dgraph_set_graph(kmx_dgraph* h, int32_t n, const double* Rrest, const double* g, int64_t m,
                         const int32_t* src, const int32_t* dst, const double* w);
/* New weights for the same edges (NULL: all 1); uploads only. When priors are
 * set the well-posedness rule is checked against them. A solve after it is
 * bitwise what a fresh handle built without the zero-weight edges gives. */
int kmx_dgraph_set_weights(kmx_dgraph* h, const double* w);
/* mode[n] (uint8), Rhat[n][3][3], that[n][3], kappa[n], tau[n]; rows of nodes
 * with mode 0 are not read. KMX_ESTATE before set_graph. */
int kmx_dgraph_set_priors(kmx_dgraph* h, const uint8_t* mode, const double* Rhat, const double* that,
                          const double* kappa, const double* tau);
/* R[n][3][3], t[n][3]; both NULL: the rest poses. */
int kmx_dgraph_set_poses(kmx_dgraph* h, const double* R, const double* t);
int kmx_dgraph_get_poses(kmx_dgraph* h, double* R, double* t);
/* At the current point, hard nodes at their priors. v: KMX_DGRAPH_EVAL_JTJ only. */
int kmx_dgraph_eval(kmx_dgraph* h, int32_t what, const double* v, double* out);
/* params NULL: every default. result may be NULL. */
int kmx_dgraph_solve(kmx_dgraph* h, const kmx_dgraph_params* params, kmx_dgraph_result* result);
/* The last solve's outer iterations: *n_out of them, the first min(cap, *n_out) written to log. */
int kmx_dgraph_get_log(kmx_dgraph* h, int32_t cap, kmx_dgraph_log_entry* log, int32_t* n_out);
/* Device times (ms, HIP events) of the last solve: [0] linearise (with the
 * preconditioner), [1] CG, [2] trial point and decision, [3] total; and [4]
 * the matrix-free product kernel alone of the last KMX_DGRAPH_EVAL_JTJ. */
int kmx_dgraph_get_timing(kmx_dgraph* h, double* ms /* [5] */);

/* ------------------------------------------------------------------------- */
/* Voxel simplification and deformation-graph build (Kimera-PGMO's stage       */
/* between the mesh and the deformation graph), csrc/simplify.hip.             */
/* ------------------------------------------------------------------------- */
/* Additive to ABI 10. An append-only handle: after any sequence of
 * kmx_simplify_add calls its arrays are those of one call with the
 * concatenated input. Every output is an integer, a copied input or a given
 * constant, so there is no tolerance.
 *  - The key of a vertex is (robot, ix, iy, iz, win): i* = floor(double(x*) /
 *    resolution), an fp64 division; win = stamp_ns / horizon_ns rounded toward
 *    minus infinity, 0 when horizon_ns is 0.
 *  - The representative of a key is the lowest vertex id that has it. Control
 *    vertices are numbered in the order of their representatives, so an append
 *    adds control ids at the end and vertex_to_control of an older vertex never
 *    changes. A control vertex carries its representative's xyz (widened to
 *    fp64), stamp and robot.
 *  - A face is mapped through vertex_to_control, dropped when two corners are
 *    equal, and of the faces with one unordered triple the one lowest in the
 *    input is kept, corner order unchanged; the kept list is append-only.
 *  - The mesh edges are the unique pairs (lo < hi) over the kept faces' sides
 *    in lexicographic order, formed on request.
 *  - The graph: nodes are the nk keyframes, then the control vertices (node
 *    nk + c). For every mesh edge in order (lo+nk -> hi+nk), (hi+nk -> lo+nk)
 *    at w_mesh; then for every control vertex c (c+nk -> link), (link -> c+nk)
 *    at w_link, link = kf_offset[a] + the first position in robot a's
 *    non-decreasing keyframe stamps whose stamp equals c's.
 * A call that returns KMX_EINVAL or KMX_EUNSUP leaves the handle as it was. */
typedef struct kmx_simplify kmx_simplify;
typedef struct {
  double resolution;     /* metres; finite and > 0 */
  int64_t horizon_ns;    /* 0: off; >= 0 */
  int32_t n_robots;      /* 1..65536 */
  int32_t initial_slots; /* of both hash tables; 0: the default (1024), a power of two otherwise */
} kmx_simplify_params;
typedef struct {
  int64_t n_vertices, n_faces_in, n_control, n_faces_kept;
  int64_t vertex_slots, face_slots; /* of the two open-addressing tables */
  int64_t device_bytes;
  int32_t vertex_rehashes, face_rehashes; /* times a table was enlarged and filled again */
  int32_t scan_span;                      /* elements one scan workgroup owns */
  int32_t scan_span2;                     /* elements one pass of the scan's second level covers */
} kmx_simplify_info_t;

int kmx_simplify_create(const kmx_simplify_params* params, int device, kmx_simplify** out);
int kmx_simplify_destroy(kmx_simplify* h);
int kmx_simplify_set_stream(kmx_simplify* h, void* hip_stream);
int kmx_simplify_sync(kmx_simplify* h);
int kmx_simplify_info(kmx_simplify* h, kmx_simplify_info_t* info);
/* Appends n_vertices vertices (robot[n], stamp_ns[n], xyz[n][3] fp32) and
 * n_faces faces (faces[n_faces][3]: vertex ids, any vertex added so far, this
 * call's included). first_vertex_out (or NULL): the id of the first new vertex;
 * counts_out (or NULL) [2]: new control vertices, new kept faces. KMX_EINVAL
 * for a null array with n > 0, a robot id out of range, a position that is not
 * finite or whose voxel index exceeds int32, a face index out of range;
 * KMX_EUNSUP for totals at or above 2^31 - 1. Returns when the result is formed. */
int kmx_simplify_add(kmx_simplify* h, int64_t n_vertices, const int32_t* robot, const int64_t* stamp_ns,
                     const float* xyz, int64_t n_faces, const int32_t* faces, int64_t* first_vertex_out,
                     int64_t* counts_out);
/* Control vertices [first, first + n): any output may be NULL. */
int kmx_simplify_get_control(kmx_simplify* h, int64_t first, int64_t n, double* xyz, int64_t* stamp_ns,
                             int32_t* robot, int32_t* representative);
int kmx_simplify_get_vertex_map(kmx_simplify* h, int64_t first, int64_t n, int32_t* vertex_to_control);
int kmx_simplify_get_faces(kmx_simplify* h, int64_t first, int64_t n, int32_t* faces /* [n][3] */);
/* Forms the unique sorted pairs on the device (once per state of the handle). */
int kmx_simplify_edges(kmx_simplify* h, int64_t* n_edges_out);
int kmx_simplify_get_edges(kmx_simplify* h, int32_t* pairs /* [n_edges][2] */);
/* kf_offset[n_robots + 1] from 0, kf_stamp[nk] robot by robot, non-decreasing
 * within a robot. *n_directed_out = 2 n_edges + 2 n_control; src, dst, w of
 * that length and link[n_control] are written when not NULL (all NULL: sizes
 * only). KMX_EINVAL for n_robots other than the handle's, a kf_offset that
 * does not start at 0 or decreases, keyframe stamps that decrease within a
 * robot, or a control vertex without a keyframe at its stamp: kmx_last_error
 * then names the lowest such robot, its count and its first such vertex. */
int kmx_simplify_graph(kmx_simplify* h, int32_t n_robots, const int64_t* kf_offset, const int64_t* kf_stamp,
                       double w_mesh, double w_link, int32_t* src, int32_t* dst, double* w, int64_t* link,
                       int64_t* n_directed_out);
/* Device times by HIP events of the last add, the last edge formation and the
 * last graph (links and emit), 0 for one that has not run; waits. */
int kmx_simplify_enable_timing(kmx_simplify* h, int enable);
int kmx_simplify_read_timing(kmx_simplify* h, double* add_ms, double* edges_ms, double* graph_ms);

#ifdef __cplusplus
}
#endif
#endif /* KMX_ABI_H */
