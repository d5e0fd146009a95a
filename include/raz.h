/* raz.h — C ABI of libraz, the MI355X-native self-play hot path that sits behind the
 * ReversiEnv / ReversiPlayer / play_*.json surface of mokemokechicken/reversi-alpha-zero.
 *
 * The reference has no FFI of its own: its seams are Python call signatures, and its only native
 * code is the Cython pair lib/alt/bitboard_cython.pyx + lib/alt/reversi_solver_cython.pyx
 * (`cpdef unsigned long long f(unsigned long long, unsigned long long)`).  Each entry point below
 * names the reference interface it replaces (file:line under /root/reference/src/reversi_zero).
 *
 * Conventions
 *   - plain C types only; device pointers are ordinary pointers into HBM owned by the CALLER
 *     (libraz never allocates or frees device memory);
 *   - `raz_stream_t` is a hipStream_t passed as void* (NULL = the null stream); batched calls are
 *     asynchronous on that stream;
 *   - functions returning int return 0 on success and a negative RAZ_E* code on failure, with a
 *     message retrievable through raz_last_error() (thread-local); nothing aborts the process;
 *   - bitboards: bit i = square i, bit 0 = top-left, bit 63 = bottom-right (lib/bitboard.py:10-17);
 *     player 1 = black, 2 = white (env/reversi_env.py:9); winner 1/2/3 = black/white/draw (:11);
 *   - an engine handle is NOT re-entrant: one host thread drives one handle on one device.
 */
#ifndef RAZ_H
#define RAZ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAZ_ABI_VERSION 3   /* 2: compact tree nodes - raz_engine_config.pool_bytes_per_game, raz_engine_stats.max_pool_bytes.
                               3: the end-game solver is a pool of worker waves shared by all games - raz_engine_config.solver_pool_waves,
                                  reserved bits 16-23 now budget the pool's launches; raz_engine_uses_graph is gone, raz_net_range_stats
                                  was added, raz_engine_config.reserved bit 2 and raz_net.reserved 5/6 are rejected */

#define RAZ_OK 0
#define RAZ_EINVAL (-1)   /* bad argument (range, NULL, alignment)            */
#define RAZ_EDEVICE (-2)  /* HIP runtime error (no device, launch failure)    */
#define RAZ_ENOMEM (-3)   /* caller-provided workspace too small              */
#define RAZ_ESTATE (-4)   /* call not valid in the handle's current state     */

typedef void* raz_stream_t;

int raz_abi_version(void);
const char* raz_last_error(void);

/* ---- scalar host primitives: lib/bitboard.py (precedent: lib/alt/bitboard_cython.pyx) -------- */
uint64_t raz_find_correct_moves(uint64_t own, uint64_t enemy);  /* bitboard.py:53  / pyx:1   */
/* bitboard.py:70 / pyx:18.  pos must be 0..63 (the reference asserts, :78): outside that range
 * the call returns 0 and records RAZ_EINVAL in raz_last_error(); the Python wrapper asserts. */
uint64_t raz_calc_flip(int pos, uint64_t own, uint64_t enemy);
int raz_bit_count(uint64_t x);                                   /* bitboard.py:132 / pyx:97  */
uint64_t raz_flip_vertical(uint64_t x);                          /* bitboard.py:119 / pyx:43  */
uint64_t raz_flip_diag_a1h8(uint64_t x);                         /* bitboard.py:141 / pyx:52  */
uint64_t raz_rotate90(uint64_t x);                               /* bitboard.py:154 / pyx:64  */
uint64_t raz_rotate180(uint64_t x);                              /* bitboard.py:158 / pyx:68  */
/* bit_to_array(x, size) (bitboard.py:136): out[i] = bit i of x, i < size <= 64. */
int raz_bit_to_array(uint64_t x, int size, uint8_t* out);

/* ReversiEnv.step (env/reversi_env.py:42-74) on one position held by the caller.
 * action 0..63, or 255 for the reference's `None` (resign).  On return *status is 0 (running) or
 * winner 1/2/3 | 0x10 (ended by an illegal no-flip move) | 0x20 (ended by resignation);
 * *legal = legal-move mask of the side to move (0 when done). */
int raz_env_step(uint64_t* black, uint64_t* white, uint8_t* player, uint8_t* status,
                 uint64_t* legal, int action);

/* ---- batched device sweeps: one board per lane over SoA arrays in HBM ----------------------- */
/* ALIGNMENT.  The kernels move two boards per lane and instruction, so the entries refuse (RAZ_EINVAL, before anything is
 * launched) arrays that are not aligned as follows; n == 0 returns RAZ_OK without looking at the pointers.
 *   the uint64_t arrays of raz_legal_moves_batch, raz_calc_flip_batch, raz_step_batch, raz_score_batch, raz_d4_batch: 16 bytes;
 *   player / status / action of raz_step_batch: 4 bytes (16 bytes for the hybrid form: see raz_sweep_forms);
 *   pos (raz_calc_flip_batch), sym (raz_d4_batch), winner / diff (raz_score_batch): 2 bytes;
 *   raz_planes_batch and raz_pick_kth_legal_batch: the natural alignment of the element types. */
/* find_correct_moves over n boards.  24 B/board. */
int raz_legal_moves_batch(const uint64_t* own, const uint64_t* enemy, uint64_t* legal, size_t n,
                          raz_stream_t stream);
/* calc_flip over n (pos, own, enemy) triples; pos[i] > 63 yields 0.  25 B/board. */
int raz_calc_flip_batch(const uint8_t* pos, const uint64_t* own, const uint64_t* enemy,
                        uint64_t* flipped, size_t n, raz_stream_t stream);
/* ReversiEnv.step over n games, in place.  Games whose status[i] != 0 on entry are finished and
 * are left untouched with legal[i] = 0 (the reference's loops never step a done env,
 * worker/self_play.py:155).  action[i] 0..63 or 255 (resign); any other value names no square and is a move that flips
 * nothing (the mover loses, status | 0x10, board untouched) on every kernel form.  45 B/board:
 * reads black,white (16) player,status,action (3); writes black,white (16) player,status (2) legal (8). */
int raz_step_batch(uint64_t* black, uint64_t* white, uint8_t* player, uint8_t* status,
                   uint64_t* legal, const uint8_t* action, size_t n, raz_stream_t stream);
/* _game_over scoring (env/reversi_env.py:76-85): winner[i] in {1,2,3} by disc count,
 * diff[i] = popcount(black) - popcount(white).  18 B/board. */
int raz_score_batch(const uint64_t* black, const uint64_t* white, uint8_t* winner, int8_t* diff,
                    size_t n, raz_stream_t stream);
/* Dihedral transform used before the net and for saved rows (agent/player.py:300-305,169-178):
 * sym[i] = flip*4 + rot, flip_vertical first, then rot right-rotations.  17 B/board. */
int raz_d4_batch(const uint64_t* in, uint64_t* out, const uint8_t* sym, size_t n,
                 raz_stream_t stream);
/* bit_to_array for the net input (agent/player.py:307-309, worker/optimize.py:225):
 * planes[i][0][sq] = bit sq of own[i], planes[i][1][sq] = bit sq of enemy[i], as float32. */
int raz_planes_batch(const uint64_t* own, const uint64_t* enemy, float* planes, size_t n,
                     raz_stream_t stream);
/* Which KERNEL FORM the whole superblocks (2048 boards) of a batch of n boards run on - large batches take the bit-sliced kernels
 * (32 boards per lane: csrc/raz_sweep_sliced.h), the rest of the batch and small batches the board-per-lane ones; results are identical.
 * The thresholds are read once per process (RAZ_SWEEP_SLICED_MIN=<boards> overrides them; RAZ_SWEEP_SLICED_STEP=0/1/2 forces the step form).
 *   *legal_moves_form: 0 = k_legal_moves (a board per lane), 1 = k_legal_moves_sliced (from 2^25 boards on);
 *   *step_form:        0 = k_step (a board per lane), 1 = k_step_sliced, 2 = k_step_hybrid (from 2^26 boards on; needs the player /
 *                      status / action arrays 16-byte aligned - a batch whose arrays are not stays on k_step).
 * For tests and benches that must know what they measured; no device work. */
int raz_sweep_forms(size_t n, int* legal_moves_form, int* step_form);
/* The largest grid, in workgroups, any sweep launch takes: 65536, or RAZ_SWEEP_MAXGRID=<workgroups> where that is lower
 * (TESTS ONLY, read once per process; unset or 0 = 65536: with a cap of 1 or 2 the kernels' grid-stride loops, the prefetch
 * pipeline of k_legal_moves / k_step and the superblock loops of the sliced kernels take several trips on some thousand boards
 * instead of 2^18 .. 2^27).  k_step_hybrid's grid is min(superblocks, RAZ_SWEEP_HYBRID_WAVES, this).  No device work. */
unsigned raz_sweep_max_grid(void);
/* Uniform random playout driver for tests/benches (test infrastructure shipped with the library,
 * mirrors SURVEY §8(c) "random playout"): action[i] = the k-th set bit of legal[i] where
 * k = rnd[i] % popcount(legal[i]); 255 when legal[i] == 0. */
int raz_pick_kth_legal_batch(const uint64_t* legal, const uint32_t* rnd, uint8_t* action, size_t n,
                             raz_stream_t stream);

/* ---- policy/value net: agent/model.py:28-72 evaluated as agent/api.py:30-45 predict() ------------
 * Weights arrive as the host-side "raznet v1" blob (int32[8] header {0x4E5A4152,1,F,R,V,3,0,0} +
 * float32 conv/dense parameters with BatchNorm folded; written by
 * reversi_alpha_zero_amd.agent.model.ReversiNet.to_blob).  The caller owns the device buffers. */
typedef struct {
    int32_t filters, res_layers, value_fc, reserved;
    void* d_weights;      /* device, >= raz_net_weight_bytes() */
    size_t weight_bytes;
} raz_net;

/* Largest value_fc the library takes: the head kernels keep (192 + value_fc) floats of the position in LDS and stay within the
 * default 64 KB of dynamic LDS a launch may use.  A wider value head is refused (raz_net_weight_bytes 0, raz_net_load RAZ_EINVAL). */
#define RAZ_NET_MAX_VALUE_FC 16192
size_t raz_net_weight_bytes(int filters, int res_layers, int value_fc); /* 0 = unsupported shape */
size_t raz_net_scratch_bytes(int filters, int value_fc, size_t n);      /* HBM scratch for n positions */
int raz_net_load(raz_net* net, const void* blob, size_t blob_bytes, void* d_weights, size_t d_bytes,
                 raz_stream_t stream);
/* ReversiModelAPI.predict (agent/api.py:30) for n positions given as (own, enemy) bitboards of the
 * side to move — the planes of agent/player.py:307-309 are formed on the fly.  policy: n x 64
 * float32 (softmax), value: n float32 (tanh).  active (nullable): positions with active[i]==0 are
 * skipped and their outputs left untouched. */
int raz_net_forward(const raz_net* net, const uint64_t* own, const uint64_t* enemy,
                    const uint8_t* active, float* policy, float* value, size_t n, void* scratch,
                    size_t scratch_bytes, raz_stream_t stream);
/* Which kernel form raz_net_forward runs a batch of n positions of `net` on (raz_net_forward takes its choice from this function):
 *   RAZ_NET_FORM_MFMA             k_net_mfma (filters 16 / 32 / 64, value_fc <= 1024; reserved 0)
 *   RAZ_NET_FORM_MFMA_WAVE        the same kernel asked for as the one-wave-per-position test variant (reserved 2)
 *   RAZ_NET_FORM_WAVE_LDS         k_net_wave, activations in LDS (reserved 1, or a shape no matrix-core kernel takes, when
 *                                 (3 * 64 * filters + 192 + value_fc) floats fit 64 KB)
 *   RAZ_NET_FORM_WAVE_SCRATCH     k_net_wave, activations in the caller's scratch (the same, when they do not fit)
 *   RAZ_NET_FORM_WIDE             k_conv0_wide + k_conv3x3_wide + k_heads_wide (filters >= 128, % 64 == 0; reserved 0 or 2)
 *   RAZ_NET_FORM_F16X3_REPAIR     raznet-forward-v2 (reserved 4) with the in-forward repair of rows out of the f16 range
 *   RAZ_NET_FORM_F16X3_NO_REPAIR  raznet-forward-v2 without it (see raz_net_range_check)
 *   RAZ_NET_FORM_F16_REPAIR       raznet-forward-v3 (reserved 8: the plain-f16 trunk, NOT within 1e-5 of the graph) on the shapes
 *                                 where v2 repairs
 *   RAZ_NET_FORM_F16_NO_REPAIR    raznet-forward-v3 on the shapes where v2 does not
 * reserved 4 and 8 take filters % 128 == 0; on a shape k_net_mfma takes they answer RAZ_NET_FORM_MFMA like 0, on any other
 * filters RAZ_EINVAL.
 * Negative (RAZ_EINVAL) for a NULL net or a `reserved` raz_net_forward refuses.  No device work. */
#define RAZ_NET_FORM_MFMA 1
#define RAZ_NET_FORM_MFMA_WAVE 2
#define RAZ_NET_FORM_WAVE_LDS 3
#define RAZ_NET_FORM_WAVE_SCRATCH 4
#define RAZ_NET_FORM_WIDE 5
#define RAZ_NET_FORM_F16X3_REPAIR 6
#define RAZ_NET_FORM_F16X3_NO_REPAIR 7
#define RAZ_NET_FORM_F16_REPAIR 8
#define RAZ_NET_FORM_F16_NO_REPAIR 9
int raz_net_form(const raz_net* net, size_t n);

/* raz_net.reserved selects the forward kernels: 0 = the exact-f32 kernels chosen by shape ("raznet-forward-v1": every output
 * one k-ordered fmaf chain, bit-identical to the CPU oracle); 4 (filters % 128 == 0) = "raznet-forward-v2": the 3x3 trunk on
 * the f16 matrix cores with every f32 operand split into two halfs (csrc/raz_net_f16x3.hip: 3 f16 MFMAs per product, f32
 * accumulation, within 1e-5 of the fp32 graph, 16/3 of the f32-MFMA rate); 1, 2: test variants of v1 (same bits).  v2's split activations must
 * stay inside the f16 range.  Where a row's f32 activations fit a CU's LDS ((2 * 64 * filters + 192 + value_fc) floats <= 160 KB:
 * filters 128, and 256 with value_fc <= 8000 - raz_net_form RAZ_NET_FORM_F16X3_REPAIR) a row (position) whose activations do not
 * is evaluated by the exact-f32 chains inside the same forward, and *overflowed = 1 reports that some forward since raz_net_load
 * had more such rows than it repairs (32; sticky).  On the other v2 shapes (RAZ_NET_FORM_F16X3_NO_REPAIR: filters >= 384, or
 * 256 with a wider value head) NO row is repaired: a single row out of range raises the sticky flag, that row's outputs cannot be
 * trusted, the other rows' can.  Either way: run the net with reserved = 0 once *overflowed = 1.  Synchronises `stream`.
 *
 * 8 (filters % 128 == 0; opt-in, never chosen for the caller) = "raznet-forward-v3": v2 with every lo half taken as zero - the
 * plain-f16 trunk, one f16 MFMA per product.  With h(x) = round-to-nearest-even of a float to f16 and S_l the per-layer power of
 * two of v2's weight image (max |w| * S_l in [2^14, 2^15)):
 *   stem             the exact-f32 chains of v1, then a = h(relu(.))
 *   trunk layer l    out = h(relu(acc * (1 / S_l) + bias [+ skip])), acc = the f32 matrix-core accumulation of h(w * S_l) * a over
 *                    all 9 * filters products (a product of two halfs is exact in f32); the skip operand is the stored f16 activation
 *   heads            the exact-f32 chains of v1 on the f16 trunk output
 * The only roundings are h() on weights and activations and the f32 accumulation: the outputs carry f16's error and are NOT
 * within 1e-5 of the fp32 graph (measured: 1.2e-3 at the worst output of a trained 256x10 net where v2 is 2e-6; 1e-2
 * on the sharp random nets of the tests).  Measured speed: 2.24 x v2's forward (11.6 against 25.9 ms for 8192 positions of the
 * 256x10 net).  It is for callers who put noise on top of the net anyway (self-play data generation);
 * evaluation against a reference stays on 0 or 4.  The weight image, the scratch size
 * and the range contract are v2's: an activation >= 60000 flags its row, which is repaired by the exact-f32 chains on the
 * RAZ_NET_FORM_F16_REPAIR shapes and raises the sticky flag on the RAZ_NET_FORM_F16_NO_REPAIR shapes, and a row's answer is a
 * function of its position alone.  raz_net_range_check and raz_net_range_stats serve it unchanged. */
int raz_net_range_check(const raz_net* net, int* overflowed, raz_stream_t stream);
/* The same plus *rows_repaired: v2 rows (positions) since raz_net_load whose activations left the f16 range and were therefore
 * evaluated by the exact-f32 chains instead, inside the forward that met them (at most 32 rows per forward; a forward with more
 * raises the sticky flag reported by *overflowed; always 0 on the RAZ_NET_FORM_F16X3_NO_REPAIR shapes).  Where rows are repaired a
 * row's answer is a function of its position alone either way.  No reference counterpart (Keras computes in fp32 throughout,
 * agent/api.py:30-45).  Synchronises `stream`. */
int raz_net_range_stats(const raz_net* net, int* overflowed, unsigned long long* rows_repaired, raz_stream_t stream);

/* ---- batched self-play engine --------------------------------------------------------------------
 * Replaces, for n_games concurrent games, SelfPlayWorker.start_game (worker/self_play.py:139-175)
 * driving two ReversiPlayer objects (agent/player.py:28-428) through ReversiEnv, with the leaf
 * evaluations of ALL live games gathered into one raz_net_forward batch per simulation step
 * (the reference batches at most prediction_queue_size=16 leaves per worker, player.py:329-355,
 * plus Pipe fan-in, api.py:75-100).  parallel_search_num simulations are in flight per game: 1 is the
 * reference's reproducible mode (SURVEY.md §7 hard part 1); 2..16 follow the reference's asyncio event
 * loop in exact virtual time (raz-sched-v1), each in-flight leaf being one row of the batch.
 *
 * Field names follow PlayConfig (config.py:128-166).  Randomness: raz-rng-v1 keyed by
 * (seed, global game id), so results do not depend on n_games, slot order or GPU count. */
typedef struct {
    int32_t thinking_loop;                    /* config.py:133 */
    int32_t required_visit_to_decide_action;  /* :134 */
    int32_t start_rethinking_turn;            /* :135 */
    int32_t change_tau_turn;                  /* :139 */
    int32_t virtual_loss;                     /* :140 (with parallel_search_num=1 only its rounding is observable) */
    int32_t allowed_resign_turn;              /* :146 */
    int32_t has_resign_threshold;             /* resign_threshold is not None */
    int32_t share_mtcs_info;                  /* share_mtcs_info_in_self_play :131 */
    int32_t mirror_updates;                   /* 1: also maintain the colour-mirrored key like player.py:279-280,
                                                 323-324 (required when share_mtcs_info=1); 0: skip those writes
                                                 (dead unless a colour-swapped transposition occurs) */
    int32_t record_root_w;                    /* 1: also record root W per ply (parity tests) */
    double c_puct;                            /* :136 */
    double noise_eps;                         /* :137 */
    double dirichlet_alpha;                   /* :138, any alpha > 0 (0.5: Box-Muller pairs; < 1 / > 1: numpy's legacy gamma schemes) */
    double resign_threshold;                  /* :145 */
    double disable_resignation_rate;          /* :147 */
    uint32_t n_games;                         /* game slots in flight (B) */
    uint32_t nodes_per_game;                  /* most tree nodes a game's pool may hold (sizes the hash table and the node directory) */
    uint32_t table_slots;                     /* hash slots per game, power of two >= 2*nodes_per_game */
    uint32_t max_plies;                       /* record capacity per game (>= 64) */
    uint32_t seed;
    uint32_t reserved;                        /* bit 0: in-kernel phase profile; bit 1: single stream; bit 3: drive even
                                                 parallel_search_num <= 1 with the slot kernel (tests); bit 4: 16-filter nets: tree and net in
                                                 ONE kernel, the game's wave evaluates its own leaves (csrc/raz_engine_fused.hip
                                                 k_tree_net / k_tree_par_net; same results); bits 8-11:
                                                 slices/streams (0 = 3); bits 12-15: max simulations per game per tree launch
                                                 (0 = 2; slot kernel: simulations STARTED per launch beyond parallel_search_num);
                                                 bits 16-23: x 64 = iterations a worker lane of the end-game solver's pool runs between two
                                                 tree launches (0 = the default, 96); a game whose solve - the root's or one inside a simulation - is
                                                 not answered yet stays suspended: results do not depend on the value;
                                                 bits 24-27: tree launches per round of that pool (0 = the library's default; 1 = every
                                                 step waits for the pool's round; n > 1 = the round runs on a stream of its own beside
                                                 the next n - 1 steps, so that games that wait for no solve are not held up by it;
                                                 raz_engine_step joins it before it returns).  Results do not depend on it either.
                                                 Every other bit must be 0 (RAZ_EINVAL) */
    int32_t use_solver_turn;                  /* config.py:154: 0 = off, else >= 46: exact end-game solve at the root
                                                 (agent/player.py:100-103,150-161; lib/alt/reversi_solver_cython.pyx) */
    int32_t use_solver_turn_in_simulation;    /* config.py:155: 0 = off, else >= 46: win/loss solve inside simulations
                                                 (agent/player.py:237-251) */
    uint32_t solver_memo_slots;               /* per-game memo of solved positions, power of two (0 with the solver off) */
    uint32_t parallel_search_num;             /* config.py:142: simulations in flight per game; 0/1 = one (the reference's
                                                 reproducible mode), 2..16 = the asyncio loop in exact virtual time
                                                 (raz-sched-v1), bit-exact vs the reference on such a loop */
    uint64_t pool_bytes_per_game;             /* bytes of a game's node pool.  Nodes are compact and variable-size: 40 B + 20 B per
                                                 LEGAL move of the position (the reference keeps three f64[64] per key = 1536 B,
                                                 agent/player.py:62-66), ~212 B on average over a game, 704 B at most.
                                                 0 = nodes_per_game x 232 + 64 x 704; at most 256 MB */
    uint32_t solver_pool_waves;               /* worker wavefronts of the end-game solver's pool (csrc/raz_solver_pool.h): positions of 5..14
                                                 empties are solved by a pool of lanes shared by all games, one subtree per lane, instead
                                                 of inside the game's own wave.  0 = one per four games, at most 1280 (what the chip's LDS holds at once); 36 KB
                                                 of workspace each.  Results do not depend on the value.  No reference counterpart
                                                 (lib/alt/reversi_solver_cython.pyx runs one position at a time) */
    uint32_t reserved2;                       /* must be 0 */
} raz_engine_config;

typedef struct raz_engine raz_engine; /* opaque host handle; not re-entrant */

typedef struct {
    uint64_t finished_games;  /* games whose status != 0 */
    uint64_t total_sims;      /* start_search_my_move invocations executed (SURVEY §8(d) metric) */
    uint64_t nn_leaves;       /* leaf positions sent to the net */
    uint64_t error_flags;     /* 0 = ok; 1 node pool full, 2 table full, 4 records full, 8 path overflow */
    uint64_t selections;      /* select_action_q_and_u calls (sum of descent depths) */
    uint64_t max_pool_used;   /* most nodes in a running game's pool (limit: nodes_per_game) */
    uint64_t idle_or_done;    /* slots that are idle (never started / one-move mode finished) or finished */
    uint64_t max_pool_bytes;  /* most bytes used in a running game's pool (limit: pool_bytes_per_game) */
} raz_engine_stats;

size_t raz_engine_workspace_bytes(const raz_engine_config* cfg);
/* d_workspace: device buffer of at least raz_engine_workspace_bytes(), 256-byte aligned, owned by
 * the caller for the lifetime of the handle.  net: loaded with raz_net_load. */
int raz_engine_create(const raz_engine_config* cfg, const raz_net* net, void* d_workspace,
                      size_t workspace_bytes, void* d_net_scratch, size_t net_scratch_bytes,
                      raz_engine** out);
void raz_engine_destroy(raz_engine* e);
/* Reset every slot to a fresh game: slot i plays global game id first_game_id + i with
 * sims_per_move[i] simulations per move (host array of n_games entries; the reference decides this
 * per game from the schedule, worker/self_play.py:145,262-272).  Slots i >= n_active stay idle. */
int raz_engine_start(raz_engine* e, uint32_t first_game_id, const uint32_t* sims_per_move,
                     uint32_t n_active, raz_stream_t stream);
/* The next game of every slot ON THE SLOT'S TREE: SelfPlayWorker.start keeps its MCTSInfo for
 * reset_mtcs_info_per_game games (worker/self_play.py:109-111,132-134; mini.yml ships 3).  Boards, records,
 * random-stream counters and statistics start afresh for global game ids first_game_id + i; nodes, tables and
 * pools stay, and every key that holds a prior counts as expanded for the new game's players
 * (agent/player.py:47).  All games of the previous round must have finished and their records been read.
 * Without share_mtcs_info the reference carries nothing over and this is raz_engine_start. */
int raz_engine_next_game(raz_engine* e, uint32_t first_game_id, const uint32_t* sims_per_move,
                         uint32_t n_active, raz_stream_t stream);
/* Enqueue n_steps simulation steps (each: tree kernel = backup + move logic + select, then one
 * net batch over the gathered leaves).  Asynchronous w.r.t. the host; all work is ordered after
 * prior work on `stream` and before later work on it.  With n_games >= 256 the batch is stepped as
 * 3 slices on `stream` and two internal streams so that one slice's net kernel overlaps the
 * other slices' tree kernels. */
int raz_engine_step(raz_engine* e, uint32_t n_steps, raz_stream_t stream);
/* Same as raz_engine_step, with HIP events recorded around every kernel launch on the stream it runs
 * on: the summed durations (ms) of the tree-kernel launches and of the net-kernel launches are
 * ADDED to *tree_ms / *net_ms (with n_games >= 256 a step is 2 launches of each kernel, one per
 * half batch, on two streams).  Synchronises the stream. */
int raz_engine_step_timed(raz_engine* e, uint32_t n_steps, double* tree_ms, double* net_ms,
                          raz_stream_t stream);
/* ReversiPlayer.action_with_evaluation(own, enemy) (agent/player.py:82-134) for the player that owns
 * slot `slot`: put the slot on (black, white, player to move) keeping its tree (the reference keeps
 * var_n/var_w/var_p across calls), its random-stream counters and its records, and arm one move of
 * `sims` simulations.  one_move != 0: the slot idles once the move is decided (read it back with
 * raz_engine_read_records: the last recorded ply); 0: the game simply continues from that position. */
int raz_engine_set_position(raz_engine* e, uint32_t slot, uint64_t black, uint64_t white, int player,
                            uint32_t sims, int enable_resign, int one_move, raz_stream_t stream);
/* raz_engine_set_position for slots first_slot .. first_slot + n - 1 in one launch: (black, white, player to move) of slot
 * first_slot + i in DEVICE arrays d_black[i], d_white[i], d_player[i] (players 1 / 2; the caller guarantees the positions are
 * playable, as with the scalar call), the same sims / enable_resign / one_move for all.  Asynchronous on `stream`. */
int raz_engine_set_positions(raz_engine* e, uint32_t first_slot, uint32_t n, const uint64_t* d_black, const uint64_t* d_white,
                             const uint8_t* d_player, uint32_t sims, int enable_resign, int one_move, raz_stream_t stream);
/* ReversiPlayer.stop_thinking (agent/player.py:163-164): the slot's running search ends at the next step
 * and the move is decided from the tree as it is. */
int raz_engine_stop_thinking(raz_engine* e, uint32_t slot, raz_stream_t stream);
/* A ReversiPlayer constructed on a used MCTSInfo takes expanded = set(var_p.keys()) (agent/player.py:47):
 * mark every key of the slot that holds a prior as expanded for player index 0/1. */
int raz_engine_adopt_tree(raz_engine* e, uint32_t slot, int player_index, raz_stream_t stream);
/* MCTSInfo introspection (agent/player.py:22,63-69: var_n[key], var_w[key], var_p[key] with
 * key = CounterKey(black, white, next_player)): copies slot `slot`'s statistics of that key into host
 * arrays of 64 (any may be NULL).  owner: 0 when share_mtcs_info, else the player index (0 black,
 * 1 white) whose tree is read.  *found = 0 and zeros (the defaultdict default) when the key was never
 * touched; the tree is not modified.  p64 is the masked, normalised prior the search uses
 * (var_p after expand_and_evaluate, player.py:283-327).  Synchronises `stream`. */
int raz_engine_read_node(raz_engine* e, uint32_t slot, uint64_t black, uint64_t white, int next_player,
                         int owner, double* w64, uint32_t* n64, float* p64, int* found, raz_stream_t stream);
/* Prune the nodes no future search can reach (positions with fewer discs than the current real
 * position; the disc count only grows) in every game whose pool holds >= threshold nodes, compacting
 * the pool and rebuilding that game's table.  Does not change any result.  Asynchronous.  A pool is full when EITHER its node
 * count reaches nodes_per_game or its bytes reach pool_bytes_per_game (error flag 1): prune when
 * max_pool_used / max_pool_bytes of raz_engine_stats_sync come close (a simulation adds at most two nodes of <= 704 B). */
int raz_engine_gc(raz_engine* e, uint32_t threshold, raz_stream_t stream);
/* Number of slices/streams a step is split into (1..8; 1 = one tree launch + one net launch over the
 * whole batch).  Call with the stream idle. */
int raz_engine_set_parts(raz_engine* e, int parts);
/* Tree launches per round of the end-game solver's pool (raz_engine_config.reserved bits 24-27 set it at creation): 0 = the library's
 * default, 1 = every step waits for the pool's round, n in 2..15 = the round runs on a stream of its own beside the next n - 1 steps.
 * A batch whose games all reach the solver together (lock-step whole games) is served best by 1, continuous batching - a sixth of
 * the slots in the end game at any time - by 3 (mini.yml as shipped, 4096 slots: 22.7 M -> 30.3 M sims/s).  No result depends on it.
 * Call between raz_engine_step calls. */
int raz_engine_set_solver_pool_every(raz_engine* e, int n);
/* Synchronise the stream and read the counters. */
int raz_engine_stats_sync(raz_engine* e, raz_engine_stats* out, raz_stream_t stream);
/* Copy finished-game records to host memory (synchronous).  headers: n_games*max_plies*48 bytes
 * (struct layout in csrc/raz_engine.h: own u64, enemy u64, n f64, q f64, action i8, player u8,
 * turn u8, has_row u8, sims u32, loops u32, pad u32); root_n: n_games*max_plies*64 u32;
 * root_w: same count of f64 or NULL; n_plies, status (winner|flags), resigned[2], game_id,
 * enable_resign: per game.  Any pointer may be NULL to skip that array. */
int raz_engine_read_records(raz_engine* e, void* headers, uint32_t* root_n, double* root_w,
                            uint32_t* n_plies, uint8_t* status, uint8_t* resigned,
                            uint32_t* game_id, uint8_t* enable_resign, uint64_t* final_black,
                            uint64_t* final_white, raz_stream_t stream);
/* The unit of the record gather ("gather of finished-game records to rank 0"): the records of slots
 * [first_slot, first_slot + n_slots), cut to `plies` plies per game (raz_engine_records_extent gives the largest
 * n_plies; unused plies are zero), packed device-to-device into dense caller arrays that a collective can move as
 * they are: d_headers n_slots*plies*48 bytes, d_root_n n_slots*plies*64 u32, d_summary n_slots raz_game_summary.
 * Asynchronous on `stream`. */
typedef struct {
    uint64_t final_black, final_white;  /* the board when the game ended */
    uint32_t game_id, n_plies;
    uint8_t status;                     /* winner | flags, as raz_env_step */
    uint8_t resigned_black, resigned_white, enable_resign;
    uint32_t sims_lo;                   /* simulations run for this game so far (low 32 bits) */
} raz_game_summary;                     /* 32 bytes */
int raz_engine_records_extent(raz_engine* e, uint32_t first_slot, uint32_t n_slots, uint32_t* max_plies,
                              raz_stream_t stream);   /* synchronises `stream` */
int raz_engine_pack_records(raz_engine* e, uint32_t first_slot, uint32_t n_slots, uint32_t plies, void* d_headers,
                            uint32_t* d_root_n, raz_game_summary* d_summary, raz_stream_t stream);
/* Continuous batching.  The reference worker starts its next game the moment one ends (worker/self_play.py:95-137); a
 * lock-step batch idles every finished slot until its slowest game is over.  raz_engine_harvest, called between
 * raz_engine_step calls: every slot whose game has finished is emptied into the caller's OUTBOX (device arrays indexed by
 * game id - out_first_id, so the outbox is in id order whatever order the games finish in: headers out_games*max_plies*48
 * bytes, root_n out_games*max_plies*64 u32, summaries, done flags set to 1) and restarted - empty tree, fresh records - on
 * the next unplayed ids next_game_id, next_game_id + 1, ... (handed to the freed slots in slot order; at most n_new_ids of
 * them, the remaining freed slots idle).  sims_per_move[k] / resign_threshold[k] (nullable; NaN = no resignation rule;
 * NULL = the engine's run-time value) are the parameters of id next_game_id + k: a game keeps the threshold it was started
 * under, so its result depends on its id and parameters only - not on the batch size, the slot, or when other games end.
 * A finished game whose id has no outbox row stays in its slot (counted in `skipped`).  Not for series of games on a
 * carried tree (raz_engine_next_game).  Synchronises `stream`. */
typedef struct {
    uint32_t harvested;   /* games moved to the outbox by this call */
    uint32_t restarted;   /* of their slots, how many started a new game (ids next_game_id .. next_game_id + restarted - 1) */
    uint32_t skipped;     /* finished games left in place: id outside the outbox */
    uint32_t playing;     /* slots with a game in progress after the call */
} raz_harvest_result;
int raz_engine_harvest(raz_engine* e, uint32_t next_game_id, uint32_t n_new_ids, const uint32_t* sims_per_move,
                       const double* resign_threshold, uint32_t out_first_id, uint32_t out_games, void* d_headers,
                       uint32_t* d_root_n, raz_game_summary* d_summary, uint8_t* d_done, raz_harvest_result* result,
                       raz_stream_t stream);
/* Cross-game evaluation cache.  The reference evaluates every leaf through the net (agent/player.py:283-327 ->
 * agent/api.py:30-45).  With thousands of games on one device the same positions are asked for again and again (every game
 * passes through the same openings; a lock-step batch searches the same roots at the same time).  The net is a pure,
 * batch-invariant function of the position, so a repeated position is served from a table - bit-identical to evaluating
 * it again: games do not change, only the number of rows the net sees.  d_cache: caller-owned device buffer of
 * raz_leaf_cache_bytes(log2_entries, n_games * max(parallel_search_num, 1)) bytes, 256-byte aligned, cleared by this call;
 * NULL detaches.  max_discs: only positions with at most that many discs on the board are looked up and stored (0 = all;
 * positions deep in a game hardly ever repeat, the openings do).  Attach a FRESH (or re-attached = cleared) cache whenever the net's weights change.  With the split-f16
 * trunk (raz_net.reserved = 4) the rows still to evaluate are compacted, so the convolutions shrink with the hit rate;
 * other nets skip the served rows through their `active` mask.  stats: out4 = {hits, duplicates inside a batch, rows
 * evaluated, claims that found no room in the table} since the cache was attached (synchronises `stream`). */
size_t raz_leaf_cache_bytes(uint32_t log2_entries, size_t rows);
int raz_engine_set_leaf_cache(raz_engine* e, void* d_cache, size_t bytes, uint32_t log2_entries, uint32_t max_discs,
                              raz_stream_t stream);
int raz_engine_leaf_cache_stats(raz_engine* e, uint64_t* out4, raz_stream_t stream);
/* Statistics of the end-game solver's pool since raz_engine_start (csrc/raz_solver_pool.h; no reference counterpart - the reference
 * solves one position at a time, lib/alt/reversi_solver_cython.pyx:40-61).  out15:
 *   [0] [1] [2] shader-clock ticks the worker waves spent in their slow phases (memo traffic + task draws) / folding finished nodes into
 *               their parents / in their loops altogether
 *   [3] solves whose task tree was built            [4] answers published
 *   [5] rounds of the pool those solves were listed in before their answer
 *   [6] lane-iterations in which a worker lane searched a subtree      [7] wave-iterations executed (x 64 = lane slots)
 *   [8] subtrees finished      [9] subtrees drawn but not searched (their node was decided already)
 *   [10] worker-wave launches that found work
 *   [11] requests posted by all game slots, [12] most by one slot
 *   [13] rounds all slots' solves were listed in, [14] most of one slot (the batch's critical path in rounds of the pool).
 * Synchronises `stream`. */
int raz_engine_solver_stats(raz_engine* e, uint64_t* out15, raz_stream_t stream);
/* ---- batched end-game solver: ReversiSolver.solve (lib/alt/reversi_solver_cython.pyx:40-127) for n positions at once ---------------
 * Independent of any engine (csrc/raz_solver_batch.hip).  Row i is (d_black[i], d_white[i], d_player[i]: 1 black / 2 white to move);
 * exactly = 0 is the reference's win/loss mode (EVERY node's loop over its moves - ascending, strict improvement - stops at the first
 * value > 0), exactly != 0 the full scan.  d_status[i]:
 *   0 solved           d_move[i] 0..63, d_score[i] the disc difference from the side to move's view: the reference's (move, score);
 *   1 no move          the side to move has no legal move - a root that must pass, a finished game, a full board: the reference's
 *                      (None, None) (:58-59);
 *   2 refused          more than 14 empty squares: not searched, never approximated;
 *   3 not a position   a square of both colours, or a player byte other than 1 / 2 (checked first): not searched;
 * rows of status 1..3 answer d_move = -1, d_score = -100.  A row's three bytes are a function of (its position, the mode) alone:
 * the other rows, n, the workspace's size, `tuning` and the stream change no output byte.
 * d_workspace: 256-byte aligned, at least raz_solve_batch_workspace_bytes(n, e) bytes where e >= the most empty squares of a row
 * that is searched (14 always suffices; 0 is returned for e > 14 and for n > 2^31: refused).  The size covers the worst case of ONE
 * row; a larger workspace lets more rows share a pass (the call cuts the batch into chunks that fit).  After the call its first 8
 * bytes hold the number of node visits (moves played) of the call, as a uint64.
 * tuning: 0 = the defaults; tests force the partition of the work with
 *   bits 0-3    leaf size: nodes with more empty squares are split into their children, smaller ones are searched by one lane
 *               (0 = 8, the largest; 2..8);
 *   bits 4-7    the most plies the leaf size above is applied for, + 1 (0 = all 6; 1 = none ... 7 = 6 plies).  Below those plies a
 *               node is split only while it has more than 8 empty squares: that much splitting is not a knob - under every tuning
 *               one lane searches a subtree of at most 8 empties (at most 109 601 node visits).  "No split" therefore means no
 *               split of positions of at most 8 empties, and no more than the bound asks for above that;
 *   bits 8-23   the most rows per chunk (0 = as many as the workspace holds);
 * any other bit, or a value outside those ranges: RAZ_EINVAL.
 * RAZ_EINVAL and NO launch: unknown tuning, a NULL or misaligned array, a workspace below raz_solve_batch_workspace_bytes(n, 0).
 * RAZ_EINVAL with no output byte written: a workspace below raz_solve_batch_workspace_bytes(n, the most empties of a searched row).
 * The call learns that number from its classification pass, so - unlike the refusals above - this one comes after that pass has been
 * launched (it writes into the workspace alone) and the stream synchronised.  RAZ_ENOMEM: no host memory for n bytes.
 * n == 0: RAZ_OK, no launch.  No GPU: RAZ_EDEVICE.
 * The call SYNCHRONISES `stream` once, after the classification pass (the host sizes the chunks from the rows' empties), and is
 * therefore not graph-capturable; the search itself is enqueued asynchronously, ordered on `stream`. */
size_t raz_solve_batch_workspace_bytes(size_t n, int max_empties);
int raz_solve_batch(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, int exactly,
                    int8_t* d_move, int8_t* d_score, uint8_t* d_status, void* d_workspace, size_t workspace_bytes,
                    uint32_t tuning, raz_stream_t stream);
/* ---- the exact solver with bounds passed down (csrc/raz_solver_exact.hip) ---------------------------------------------------------
 * raz_solve_batch(..., exactly = 1, ...) for positions of up to RAZ_SOLVE_EXACT_MAX_EMPTIES empty squares: row i answers exactly what
 * raz_solve_batch answers in its full-scan mode for every row both accept - the game-theoretic disc difference from the side to
 * move's view, and the lowest-numbered legal move that attains it - found by a depth-first search that passes bounds down
 * (alpha-beta) instead of the exhaustive scan.  Status codes 0 / 1 / 2 / 3, d_move = -1 and d_score = -100 where status != 0, as
 * above; status 2 (refused) now means more than RAZ_SOLVE_EXACT_MAX_EMPTIES empties.  There is no win/loss mode here.  A row's three
 * bytes are a function of its position alone: the other rows, n, the workspace's size, `tuning` and the stream change no output byte.
 * d_workspace: 256-byte aligned, at least raz_solve_exact_workspace_bytes(n, e) bytes where e >= the most empties of a searched row
 * (0 is returned for e > RAZ_SOLVE_EXACT_MAX_EMPTIES and for n > 2^31: refused).  That size holds the default split of one row and
 * the parked stacks of the lanes that search; with more, more rows share a pass.  After the call its first 8 bytes hold the call's
 * node visits (moves played), as a uint64 - a number that, unlike the outputs, depends on the order in which lanes finish.
 * The search runs in ROUNDS: in one launch no lane visits more than the node budget; a lane that runs out parks its stack in the
 * workspace and resumes in the next launch.  The host ends the rounds when the device reports nothing left, and returns
 * RAZ_EDEVICE if that has not happened after the number of rounds the bound on the chunk's node visits allows, or as soon as a
 * group of rounds neither visited a node nor drew a record.
 * tuning: 0 = the defaults; tests force the partition of the work with
 *   bits 0-4    leaf size: during the split plies a node with more empties gets its children as tasks (0 = 10; 2..17);
 *   bits 5-7    the most plies the leaf size is applied for, + 1 (0 = all 6; 1 = none ... 7 = 6 plies).  Below those plies a node
 *               is split only while it has more than 12 empty squares: that much splitting is not a knob - under every tuning one
 *               lane's task is a subtree of at most 12 empties;
 *   bits 8-19   the most rows per chunk (0 = as many as the workspace holds);
 *   bits 20-23  the node budget of a lane per launch: 0 = 32 768, 1 = 3, 2 = 16, 3 = 128, 4 = 1 024, 5 = 8 192;
 *   bit 24      children are searched in ascending order (no ordering by the opponent's mobility);
 *   bit 25      tasks do not share their parent's bound (every task is searched under the full window);
 * any other bit, or a value outside those ranges: RAZ_EINVAL.
 * RAZ_EINVAL and NO launch: unknown tuning, a NULL or misaligned array, a workspace below raz_solve_exact_workspace_bytes(n, 0).
 * RAZ_EINVAL with no output byte written: a workspace below raz_solve_exact_workspace_bytes(n, the most empties of a searched row);
 * as with raz_solve_batch this one comes after the classification pass.  RAZ_ENOMEM: no host memory for n bytes.
 * n == 0: RAZ_OK, no launch.  No GPU: RAZ_EDEVICE.
 * The call SYNCHRONISES `stream` once after the classification pass and once after every GROUP of rounds of every chunk (1, 2, 4 ... 16
 * launches; the host reads whether anything is left), and is therefore not graph-capturable; when it returns, the outputs are enqueued on `stream`. */
#define RAZ_SOLVE_EXACT_MAX_EMPTIES 17
size_t raz_solve_exact_workspace_bytes(size_t n, int max_empties);
int raz_solve_exact(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, int8_t* d_move,
                    int8_t* d_score, uint8_t* d_status, void* d_workspace, size_t workspace_bytes, uint32_t tuning,
                    raz_stream_t stream);
/* ---- the win / draw / loss solver (csrc/raz_solver_wld.hip) -----------------------------------------------------------------------
 * WHO WINS, for positions of up to RAZ_SOLVE_WLD_MAX_EMPTIES empty squares.  The argument list and every convention of
 * raz_solve_exact carry over: status codes 0 / 1 / 2 / 3 (2 = more than RAZ_SOLVE_WLD_MAX_EMPTIES empties), d_move = -1 and
 * d_score = -100 where status != 0, the refusals and what they leave unwritten, n == 0, the node-visit counter in the first 8 bytes
 * of the workspace, the rounds, their groups and the caps on them, the synchronisations.  A solved row answers
 *   d_score[i]  the OUTCOME o: +1, 0 or -1 - the sign of the game-theoretic disc difference from the side to move's view, under
 *               ReversiEnv's rules (disc count only);
 *   d_move[i]   the lowest-numbered legal move whose own outcome for the mover equals o.
 * Both are functions of the position alone: the other rows, n, the workspace's size, `tuning` and the stream change no output byte.
 * This is not the move raz_solve_exact returns (the lowest-numbered move of the best DISC DIFFERENCE), nor raz_solve_batch's
 * exactly = 0 scan.
 * d_workspace: 256-byte aligned, at least raz_solve_wld_workspace_bytes(n, e) bytes where e >= the most empties of a searched row
 * (0 is returned for e > RAZ_SOLVE_WLD_MAX_EMPTIES and for n > 2^31: refused).  That size holds the default split of one row in the
 * worst case - six plies down to 10 empties, and in any case down to 15: at 21 empties 41 664 022 records of 44 bytes, 1.83 GB - and the
 * parked stacks of the lanes that search.
 * tuning: raz_solve_exact's word -
 *   bits 0-4    leaf size (0 = 10; 2..RAZ_SOLVE_WLD_MAX_EMPTIES);
 *   bits 5-7    the most plies the leaf size is applied for, + 1 (0 = all 6).  Below those plies a node is split only while it has
 *               more than 15 empty squares: under every tuning one lane's task is a subtree of at most 15 empties;
 *   bits 8-19   the most rows per chunk (0 = as many as the workspace holds);
 *   bits 20-23  the node budget of a lane per launch: 0 = 1 024, 1 = 3, 2 = 16, 3 = 128, 4 = 1 024, 5 = 8 192, 6 = 32 768;
 *   bit 24      children are searched in ascending order (no ordering by the opponent's mobility);
 *   bit 25      a task's window is not narrowed by what its ancestors have proven (it is still dropped where one is decided);
 *   bit 26      record cuts off: no task looks at its ancestors, none is dropped, nothing is reported upward;
 * any other bit, or a value outside those ranges: RAZ_EINVAL. */
#define RAZ_SOLVE_WLD_MAX_EMPTIES 21
size_t raz_solve_wld_workspace_bytes(size_t n, int max_empties);
int raz_solve_wld(const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player, size_t n, int8_t* d_move,
                  int8_t* d_score, uint8_t* d_status, void* d_workspace, size_t workspace_bytes, uint32_t tuning,
                  raz_stream_t stream);
/* Diagnostics (no reference counterpart): `bytes` at `offset` of one of the engine's device arrays (raz_engine_device_ptr's numbering:
 * 3 the games' control blocks, 6 the solver blocks, 7 / 8 / 9 the solver pool's lane state / headers / active list) copied to host
 * memory.  RAZ_EINVAL when offset + bytes reaches beyond the array.  Synchronises the device. */
int raz_engine_debug_read(raz_engine* e, int which, size_t offset, size_t bytes, void* host_out);
/* Diagnostics: the device forms of raz-math-v1 / raz-rng-v1 (csrc/raz_detmath.h) and of the wave-level reductions of the tree
 * kernels (csrc/raz_engine_core.h) applied to n elements / rows - the very functions the tree kernels call, so that a test can
 * compare them with the oracle and with numpy on inputs no game reaches.  All buffers are DEVICE buffers, rows are 64 wide
 * (lane = column); asynchronous on `stream`.  what, in0, in1 (NULL where "-") -> out:
 *   PHILOX           u32[n][6] c0..c3,k0,k1                    -                  u32[n][4]
 *   RNG_PAIR         u32[n][6] seed,game,purpose,event,sub,idx -                  f64[n][2]
 *   LOG, EXP, COS2   f64[n]                                    -                  f64[n]
 *   POW              f64[n] x                                  f64[n] y           f64[n]
 *   EXPF, TANHF      f32[n]                                    -                  f32[n]
 *   GAMMA_HALF_PAIR  u32[n][4] seed,game,event,m               -                  f64[n][2]
 *   GAMMA_ATTEMPT    f64[n] alpha                              u32[n][5] seed,game,event,sub,t   f64[n][2] X, accepted (0.0 / 1.0)
 *   NP_SUM_F32       f32[n][64]                                -                  f32[n]
 *   ARGMAX_F64, ARGMAX_NONNEG_F64   f64[n][64]                 -                  i32[n]   (NONNEG: finite values >= +0 only)
 *   MAX_F64          f64[n][64]                                -                  f64[n]
 *   SUM_U32          u32[n][64]                                -                  u32[n]
 *   ROOT_GAMMAS      f64[n] alpha                              u32[n][4] k,seed,game,event
 *                    -> f64[n][64] Gamma samples by rank, then f64[n][64] the normalised noise, then u32[n] rounds of the rejection
 *                    loop (0 at alpha = 0.5), one after the other in `out` ((1024 + 4) n bytes); a row whose k is outside 1..64 or
 *                    whose alpha is not a finite number > 0 is answered with zeros
 *   CHOICE           f64[n][64] policy                         f64[n] uniform     i32[n]
 * RAZ_EINVAL for an unknown selector, a missing buffer or n >= 2^24 rows of a 64-wide selector. */
#define RAZ_PROBE_PHILOX 0
#define RAZ_PROBE_RNG_PAIR 1
#define RAZ_PROBE_LOG 2
#define RAZ_PROBE_EXP 3
#define RAZ_PROBE_COS2 4
#define RAZ_PROBE_POW 5
#define RAZ_PROBE_EXPF 6
#define RAZ_PROBE_TANHF 7
#define RAZ_PROBE_GAMMA_HALF_PAIR 8
#define RAZ_PROBE_GAMMA_ATTEMPT 9
#define RAZ_PROBE_NP_SUM_F32 10
#define RAZ_PROBE_ARGMAX_F64 11
#define RAZ_PROBE_ARGMAX_NONNEG_F64 12
#define RAZ_PROBE_MAX_F64 13
#define RAZ_PROBE_SUM_U32 14
#define RAZ_PROBE_ROOT_GAMMAS 15
#define RAZ_PROBE_CHOICE 16
int raz_spec_probe(int what, const void* in0, const void* in1, void* out, size_t n, raz_stream_t stream);
/* Diagnostics: the evaluation cache's own claim / resolve / fill kernels (csrc/raz_leaf_cache.hip) on caller-supplied DEVICE buffers,
 * with no engine and no net - the functions raz_engine_step calls around the net forward of one slice, so that a test can put
 * positions no game reaches in front of them (equal tags with different keys, a full probe window, a window that wraps, claims left
 * unfinished).  phase 0 clears the table as raz_engine_set_leaf_cache does; phase 1 is the half before the forward of rows
 * [p0, p0 + pn) (claim, then resolve: hits are answered and leave `d_active`, in-batch duplicates leave it and wait, the rest are
 * listed); phase 2 the half after it (fill: owners publish their answer, waiting rows copy their owner's).  `part` is the slice's
 * number (its row count is n_compact[part]), `step` the value the engine's cache_step has for that step (it starts at 1: a cleared
 * stamp never equals a live step).  max_discs: 0 = 64, as in raz_engine_set_leaf_cache.  d_own / d_enemy u64[rows], d_active
 * u8[rows], d_policy f32[rows][64], d_value f32[rows].  Asynchronous on `stream`.
 * d_cache: raz_leaf_cache_bytes(log2_entries, rows) bytes, 256-byte aligned.  Its sections, in this order, each rounded up to a
 * multiple of 256 bytes (E = 2^log2_entries):
 *   tags u64[E] (0 = empty, else the position's hash | 1), keys u64[E][2] (own, enemy), stamp u32[E], owner u32[E], ready u32[E],
 *   pv f32[E][72] (policy 64, value, 7 words of padding), counters u64[8] ([0..3] as raz_engine_leaf_cache_stats),
 *   n_compact u32[16], list u32[rows] (a slice's rows still to evaluate, RELATIVE to p0, from list[p0] on), role u32[rows]
 *   (entry << 3 | kind; kind 0 none, 1 plain, 2 owner of the entry, 4 waiting for the entry's owner).
 * RAZ_EINVAL and NO launch: an unknown phase, log2_entries outside 10..28, `bytes` below raz_leaf_cache_bytes, a NULL or misaligned
 * buffer, p0 + pn > rows, part >= 16, pn == 0 in phase 1 or 2. */
int raz_leaf_cache_probe(int phase, void* d_cache, size_t bytes, uint32_t log2_entries, uint32_t max_discs, size_t rows,
                         const uint64_t* d_own, const uint64_t* d_enemy, uint8_t* d_active, float* d_policy, float* d_value,
                         uint32_t p0, uint32_t pn, uint32_t part, uint32_t step, raz_stream_t stream);
/* config.play.resign_threshold is mutated while the worker runs (worker/self_play.py:250-260: +-0.01 per 100
 * no-resign test games); moves decided from the next raz_engine_step on use the new value.  Trees, records and
 * random streams are untouched. */
int raz_engine_set_resign_threshold(raz_engine* e, int has_threshold, double threshold);
/* The play_*.json text of ONE finished game, natively: the rows SelfPlayWorker.save_play_data appends for it
 * (worker/self_play.py:180-194: black.moves + white.moves; agent/player.py:166-179: 8 symmetric rows
 * [[own, enemy], [64 floats]] per searched ply, :357-364: z appended; saved policy per :132,366-385), as the
 * exact bytes json.dump would write for them - rows joined by ", ", WITHOUT the enclosing "[" "]" of the file
 * (a file is "[" + the fragments of its games joined by ", " + "]").  headers / root_n: n_plies records as
 * raz_engine_read_records returns them for that game; winner: status & 0x0f.  Host function, thread-safe.
 * Returns the number of bytes written (0 for a game without rows), negative on error (RAZ_ENOMEM: cap too
 * small - 8 x 2048 bytes per ply always suffice); *n_rows (nullable) receives the number of rows. */
long long raz_emit_game_rows_json(const void* headers, const uint32_t* root_n, int n_plies, int winner,
                                  int change_tau_turn, int save_policy_of_tau_1, char* out, size_t cap,
                                  int* n_rows);
/* float.__repr__(x) (the number format of json.dump) into out32 (>= 32 bytes, NUL-terminated); returns its length. */
int raz_format_float_repr(double x, char* out32);
/* Device pointers of the engine's arrays, for a caller that gathers / inspects them itself (e.g. RCCL): which = 0 ply headers, 1 root_n,
 * 2 root_w (NULL unless record_root_w), 3 the games' control blocks, 5 the phase profile, 6-9 the solver pool (diagnostics);
 * 10-14 the LEAF EXCHANGE with the net - the role of the reference's prediction queue (agent/player.py:329-346, agent/api.py:30-45):
 * one row per simulation slot (row = game * parallel_search_num + slot): 10 active u8 (1 = the last step's net forward evaluated the
 * row; rows served by the evaluation cache read 0), 11 own u64, 12 enemy u64 (the position as shown to the net, D4 transform
 * applied), 13 policy f32[64], 14 value f32 - what the net answered.  NULL for any other number. */
void* raz_engine_device_ptr(raz_engine* e, int which);

/* ---- raznet-train-v1: one training step of the net on the device (worker/optimize.py:73-86) ---------------
 * The trainer holds the UNFOLDED graph of agent/model.py:28-72 in caller-owned device memory: parameters, Keras SGD momentum
 * buffers, BatchNorm moving statistics, the saved tensors of one batch of at most max_batch rows and the partial sums of the
 * ordered reductions.  Exact f32; the three 3x3 products of every trunk layer run on v_mfma_f32_16x16x4_f32.  No floating-point
 * atomics: the same state and batches give the same bytes.  One device, one stream at a time, not re-entrant.
 * Shapes: filters % 16 == 0 within 16..1024, cnn_filter_size 3, value_fc 1..16192, max_batch 1..65536; anything else:
 * raz_trainer_bytes / raz_trainer_state_bytes 0, raz_trainer_create RAZ_EINVAL.
 * THE TRAIN BLOB (raz_trainer_set_state / _get_state; f32, raz_trainer_state_bytes): parameters | moving statistics | momentum.
 *   parameters: for every Conv2D + BatchNormalization pair in creation order (stem, the 2 R trunk layers, policy conv, value conv)
 *     kernel [out][in][kh][kw], bias [out], gamma [out], beta [out]; then policy_out kernel [128][64] (in, out), bias [64];
 *     dense_1 kernel [64][V], bias [V]; value_out kernel [V], bias [1];
 *   moving statistics: per pair moving_mean [out], moving_variance [out];   momentum: as the parameters.
 * The data set stays packed on the device (8 + 8 + 256 + 1 bytes per row): d_own / d_enemy u64[N], d_policy f32[N][64], d_z i8[N];
 * d_idx u32[batch] names the rows of the batch.  AN INDEX >= N IS THE CALLER'S CONTRACT: it is not checked and reads out of bounds.
 * raz_trainer_step: forward in training mode (batch statistics; moving statistics updated with momentum 0.99), the gradients of
 *   mean_b sum_a -pi log(p + 1e-7) + mean_b (v - z)^2 + l2 sum w^2 over the Conv2D / Dense kernels (gradient term 2 l2 w), then
 *   m <- 0.9 m - lr g, w <- w + m.  d_losses f32[2] receives the policy and the value loss of the batch (before the update).
 * raz_trainer_backward: the same without the update of parameters, momentum and moving statistics; the gradients stay in the trainer.
 * raz_trainer_read (device to device, ordered on `stream`; `bytes` must be the tensor's size) of the LAST step / backward:
 *   RAZ_TRAIN_READ_GRADS   f32, the parameters' order and size (conv biases ahead of BatchNorm are exactly 0)
 *   RAZ_TRAIN_READ_ACT     the post-ReLU output [batch][out][64] of pair `layer` (0 stem .. 2 R trunk, 2 R + 1 policy, 2 R + 2 value)
 *   RAZ_TRAIN_READ_MEAN / _VAR   batch mean / biased batch variance [out] of pair `layer`
 *   RAZ_TRAIN_READ_HIDDEN  dense_1's post-ReLU output [batch][V];  _POLICY the softmax [batch][64];  _VALUE the tanh [batch]
 * RAZ_EINVAL and NO launch, state untouched: a NULL trainer or array, d_own / d_enemy not 8-byte or d_policy / d_idx / d_losses not
 * 4-byte aligned, batch == 0 or > max_batch, a workspace that is NULL, not 256-byte aligned or below raz_trainer_bytes, a state
 * or read size that does not match. */
typedef struct raz_trainer raz_trainer;
#define RAZ_TRAIN_READ_GRADS 0
#define RAZ_TRAIN_READ_ACT 1
#define RAZ_TRAIN_READ_MEAN 2
#define RAZ_TRAIN_READ_VAR 3
#define RAZ_TRAIN_READ_HIDDEN 4
#define RAZ_TRAIN_READ_POLICY 5
#define RAZ_TRAIN_READ_VALUE 6
size_t raz_trainer_bytes(int filters, int res_layers, int value_fc, size_t max_batch);
size_t raz_trainer_state_bytes(int filters, int res_layers, int value_fc);
int raz_trainer_create(int filters, int res_layers, int value_fc, size_t max_batch, void* d_workspace, size_t workspace_bytes,
                       raz_trainer** out, raz_stream_t stream);
void raz_trainer_destroy(raz_trainer* t);
int raz_trainer_set_state(raz_trainer* t, const float* d_blob, size_t bytes, raz_stream_t stream);
int raz_trainer_get_state(raz_trainer* t, float* d_blob, size_t bytes, raz_stream_t stream);
int raz_trainer_step(raz_trainer* t, const uint64_t* d_own, const uint64_t* d_enemy, const float* d_policy, const int8_t* d_z,
                     const uint32_t* d_idx, size_t batch, float lr, float l2, float* d_losses, raz_stream_t stream);
int raz_trainer_backward(raz_trainer* t, const uint64_t* d_own, const uint64_t* d_enemy, const float* d_policy, const int8_t* d_z,
                         const uint32_t* d_idx, size_t batch, float l2, float* d_losses, raz_stream_t stream);
int raz_trainer_read(raz_trainer* t, int which, int layer, void* d_out, size_t bytes, raz_stream_t stream);
/* raznet-train-v2, opt-in: the same step, train blob and fixed summation orders with the three 3x3 products
 * of every trunk layer on the f16 matrix cores - every f32 operand as two halfs under a per-tensor power-of-two scale, three
 * v_mfma_f32_32x32x16_f16 per product into one f32 accumulator, un-scaled once.  precision RAZ_TRAIN_F32: raz_trainer_bytes /
 * raz_trainer_create to the byte; RAZ_TRAIN_F16X3: v2 (a larger workspace; reproducible, but not v1's bytes); any other value:
 * raz_trainer_bytes2 returns 0 and raz_trainer_create2 RAZ_EINVAL, both with a message.  raz_trainer_precision: what a trainer was
 * created with (RAZ_EINVAL for NULL).  Every other entry takes either kind of trainer. */
#define RAZ_TRAIN_F32 0
#define RAZ_TRAIN_F16X3 1
size_t raz_trainer_bytes2(int filters, int res_layers, int value_fc, size_t max_batch, int precision);
int raz_trainer_create2(int filters, int res_layers, int value_fc, size_t max_batch, int precision, void* d_workspace,
                        size_t workspace_bytes, raz_trainer** out, raz_stream_t stream);
int raz_trainer_precision(const raz_trainer* t);

/* ---- training rows on the device: the self-play outbox as the trainer's packed data set (csrc/raz_replay.hip) ------
 * The rows raz_emit_game_rows_json writes as text and the `opt` worker reads back (worker/self_play.py:180-194,219-231: black.moves +
 * white.moves, z by the winner; agent/player.py:166-179: 8 symmetric rows per searched ply, :132,366-385: the saved policy;
 * worker/optimize.py:214-231: the consumer), without the text: d_own u64[R], d_enemy u64[R], d_policy f32[R][64], d_z i8[R] - the layout
 * raz_trainer_step takes - bit for bit what json.load and lib/data_helper.pack_game_data make of the files.
 * Inputs: the arrays raz_engine_pack_records and raz_engine_harvest fill - d_headers [n_games][plies] ply headers of 48 bytes, d_root_n
 * [n_games][plies][64], d_summary [n_games], d_done (nullable) [n_games] - in game order.  For a game with winner = status & 0x0f:
 *   rows    8 for every ply j < min(n_plies, plies) with has_row and player 1 or 2; none where d_done is given and d_done[g] == 0;
 *   order   the plies of player 1 in ply order, then those of player 2; within a ply flip in {0, 1} major, rot in 0..3 minor;
 *   boards  flip_vertical (if flip), then rot x rotate90, on own and on enemy;
 *   policy  output square i takes source square policy_permutation(flip, rot)[i] (np.flipud, then np.rot90(k=-rot)) of: with
 *           save_policy_of_tau_1 or turn < change_tau_turn, (float)((double)n[i] / (double)sum(n)) - the exact integer sum, which may
 *           pass 2^32, ONE f64 division, one rounding to f32 (sum == 0: the plain division); otherwise 1.0 at the first maximum of n
 *           (unsigned compare, lowest square on ties) and 0.0 elsewhere;
 *   z       black's rows +1 / -1 / 0 for winner 1 / 2 / anything else, white's rows the negative.
 * raz_train_rows_count: d_row_offset u32[n_games + 1] receives the exclusive prefix sum of the games' row counts in game order, the
 *   total at [n_games]; computed on the device in one fixed order, without atomics.  total_rows (host, nullable) receives the total;
 *   non-NULL SYNCHRONISES `stream`.  n_games == 0: RAZ_OK, d_row_offset[0] = 0 (the other arrays are not looked at).
 * raz_train_rows_fill: row d_row_offset[g] + 8 x (rank of the ply in the order above) + flip * 4 + rot.  No row >= capacity_rows is
 *   touched, in any array, and nothing at all for a game without rows.  Asynchronous on `stream`.  n_games == 0: RAZ_OK.
 * RAZ_EINVAL with a message and NO launch: a NULL array (d_done excepted), d_headers / d_summary / d_own / d_enemy not 8-byte or
 * d_root_n / d_row_offset / d_policy not 4-byte aligned, plies == 0, n_games x plies x 8 >= 2^32 (row numbers are 32-bit).  No GPU:
 * RAZ_EDEVICE. */
int raz_train_rows_count(const void* d_headers, const raz_game_summary* d_summary, const uint8_t* d_done, uint32_t n_games,
                         uint32_t plies, uint32_t* d_row_offset, uint64_t* total_rows, raz_stream_t stream);
int raz_train_rows_fill(const void* d_headers, const uint32_t* d_root_n, const raz_game_summary* d_summary, const uint8_t* d_done,
                        uint32_t n_games, uint32_t plies, int change_tau_turn, int save_policy_of_tau_1,
                        const uint32_t* d_row_offset, uint64_t capacity_rows, uint64_t* d_own, uint64_t* d_enemy, float* d_policy,
                        int8_t* d_z, raz_stream_t stream);

/* ---- evaluation matches on the device: the hand-off between two engines (csrc/raz_match.h, raz_handoff.h) --------
 * The reference's evaluator (worker/evaluate.py:66-96) plays best model against challenger with two ReversiPlayer objects and one
 * ReversiEnv per game.  A match couples two STARTED engines of the same n_games - slot g of each is that model's player in game g,
 * with the tree, random streams and one-move semantics raz_engine_set_position gives it - and keeps every game's env in a
 * caller-provided device workspace (raz_match_workspace_bytes(n_games) bytes, 256-byte aligned, owned by the caller, as are the
 * engines, for the lifetime of the handle; 0 is returned for n_games == 0):
 *   raz_match_stats u32[8] | raz_match_game [n_games] | raz_match_ply [n_games][64] | root visit counts u32 [n_games][64][64],
 *   each section rounded up to 256 bytes.
 * raz_match_start: game g is (d_black[g], d_white[g], d_player[g] 1 black / 2 white to move) - the three arrays are nullable, all or
 *   none: NULL = the initial position, black to move; the caller guarantees playable positions, as with raz_engine_set_positions -
 *   and the best model plays black where d_best_is_black[g] != 0.  One launch clears the log and arms the side to move of every game
 *   in its model's engine: the mover's own discs as "black", player 1, sims_best / sims_challenger simulations, one move.
 * raz_match_turn: one launch over all games.  A live game whose searching slot has decided (phase idle, one ply recorded) gets the
 *   ply appended to its log (who, action, turn, the 64 root visit counts), its board and status translated from the mover's frame to
 *   absolute colours, and either its outcome stored or the next mover's slot armed - the other engine's, or the same one again when
 *   the opponent had to pass.  A game whose slot is still searching is left alone.  A slot that carries an engine error flag, or that
 *   left the one-move protocol, ends its game and marks `error` (the engine's flags; RAZ_MATCH_ERR_SLOT / _LOG_FULL): a match never
 *   spins.
 * raz_match_stats_sync: the counters (synchronises `stream`).  raz_match_read: the games and, optionally, the log, to host arrays of
 *   n_games, n_games x 64 and n_games x 64 x 64 entries (any may be NULL; synchronises `stream`).
 * RAZ_EINVAL / RAZ_ESTATE with a message and NO launch: a NULL argument, engines of different n_games or not started, a workspace that
 *   is NULL, misaligned or short, sims of 0, position arrays given in part, turn / read before start. */
typedef struct raz_match raz_match;
typedef struct {
    uint64_t black, white;       /* the real board, absolute colours */
    uint8_t player;              /* side to move: 1 black / 2 white */
    uint8_t best_is_black;
    uint8_t searching;           /* whose slot is searching: 0 nobody (the game has ended), 1 the best model's, 2 the challenger's */
    uint8_t winner;              /* 0 running; 1 black / 2 white / 3 draw */
    uint8_t blacks, whites;      /* disc counts when the game ended */
    uint8_t n_plies;             /* entries of the game's log */
    uint8_t flags;               /* 0x10 ended by an illegal move, 0x20 by a resignation (as raz_env_step) */
    uint32_t pad[2];
} raz_match_game;                /* 32 bytes */
typedef struct {
    uint8_t who;                 /* 0 the best model moved, 1 the challenger */
    int8_t action;               /* 0..63, -1 = resigned */
    uint8_t turn, pad;
} raz_match_ply;                 /* 4 bytes */
typedef struct {
    uint32_t live;               /* games still running */
    uint32_t searching_best, searching_challenger;   /* slots searching per side */
    uint32_t plies;              /* plies handed off since raz_match_start */
    uint32_t error;              /* 0, or engine error flags of a slot (1 pool, 2 table, 4 records, 8 path) | RAZ_MATCH_ERR_* */
    uint32_t pad[3];
} raz_match_stats;               /* 32 bytes */
#define RAZ_MATCH_ERR_SLOT 0x100u       /* a searching slot finished outside the one-move protocol (phase done, or idle without exactly one ply) */
#define RAZ_MATCH_ERR_LOG_FULL 0x200u   /* a game's 65th ply */
#define RAZ_MATCH_MAX_PLIES 64
size_t raz_match_workspace_bytes(uint32_t n_games);
int raz_match_create(raz_engine* best_engine, raz_engine* challenger_engine, void* d_workspace, size_t workspace_bytes,
                     raz_match** out);
void raz_match_destroy(raz_match* m);
int raz_match_start(raz_match* m, const uint8_t* d_best_is_black, const uint64_t* d_black, const uint64_t* d_white,
                    const uint8_t* d_player, uint32_t sims_best, uint32_t sims_challenger, int enable_resign, raz_stream_t stream);
int raz_match_turn(raz_match* m, raz_stream_t stream);
int raz_match_stats_sync(raz_match* m, raz_match_stats* out, raz_stream_t stream);
int raz_match_read(raz_match* m, raz_match_game* games, raz_match_ply* log, uint32_t* log_root_n, raz_stream_t stream);

/* ---- retrograde analysis of whole games on the device (csrc/raz_analysis.h) ----------------------------------------
 * The NBoard command the reference leaves as `pass` (play_game/nboard.py:321-330: "for each board position occurring in the game the
 * engine sends back ... {movesMade} {eval}"), for n_games games at once.  Game g is a start position and a list of at most max_moves
 * entries; P = max_moves + 1; position (g, j) is the position after j entries and belongs to slot first_slot + g * P + j of ONE started
 * engine created with record_root_w, which searches it with the tree, random streams and one-move semantics
 * raz_engine_set_position gives that slot.  The caller steps the engine.  The analysis lives in a caller-provided device workspace
 * (raz_analysis_workspace_bytes(n_games, max_moves) bytes, 256-byte aligned, owned by the caller, as is the engine, for the lifetime
 * of the handle; 0 is returned for n_games == 0 or max_moves outside 1..127):
 *   raz_analysis_stats u32[8] | raz_analysis_game [n_games] | raz_analysis_pos [n_games][P] | raz_analysis_eval [n_games][P],
 *   each section rounded up to 256 bytes.
 * raz_analysis_start: game g starts on (d_black[g], d_white[g], d_player[g] 1 black / 2 white to move) - the three arrays are
 *   nullable, all or none: NULL = the initial position, black to move; the caller guarantees playable positions - and plays
 *   d_moves[g][0 .. max_moves): 0..63 a move, -1 a pass entry ("PA"), -2 the end of the list; any other value ends the list and sets
 *   RAZ_ANALYSIS_ERR_BAD_CODE in the game's summary and the stats.  One launch, one thread per game, clears the workspace and walks
 *   every list as NBoardEngine.set_game does (nboard.py:96-103: env.update, then env.step(action) for every entry that is not a pass
 *   entry) under ReversiEnv.step's rules (env/reversi_env.py:42-104: the automatic pass, game over when neither side can move,
 *   illegal_move_to_lose on a move that flips nothing).  It writes the position before every entry, the game's summary, and arms the
 *   slot of every SEARCH position: the mover's own discs as "black", player 1, `sims` simulations, one move, no resignation
 *   (nboard.py:50).  Every other slot of the range is left untouched.  Entries after the game is over are IGNORED - the reference
 *   would go on stepping a finished env; that is not reproduced.
 * raz_analysis_collect: one launch, one wave per position.  A pending position whose slot has decided (phase idle, one ply recorded -
 *   raz_match_turn's rule) gets its eval: the engine's action, the sum of the root's visit counts, the up to RAZ_ANALYSIS_TOP squares
 *   with n > 0 by visit count descending (lowest square first among equals) with n and q = w / ((double)n + 1e-5)
 *   (ReversiPlayer.var_q, agent/player.py:62-64), and the same pair for the entry played from the position (0, 0.0 where that is no
 *   move).  A slot the root solver answered (ply header flag bit 0) gives state SOLVED and ONE entry: the action with the header's
 *   exact n and q (sum_n = that n; the played pair is that pair where the entry is the action, else 0, 0.0).  A slot still searching
 *   is left pending.  A slot that carries an engine error flag, or that left the one-move protocol, gives state ERROR and ORs the
 *   flags / RAZ_ANALYSIS_ERR_SLOT into the stats' error word: an analysis never spins.  A position already collected is not written
 *   again, and no position waits for another.
 * raz_analysis_stats_sync: the counters (synchronises `stream`).  raz_analysis_read: the games, positions and evals to host arrays of
 *   n_games, n_games x P and n_games x P entries (any may be NULL; synchronises `stream`).
 * RAZ_EINVAL / RAZ_ESTATE with a message and NO launch: a NULL argument, an engine that is not started or was created without
 *   record_root_w, first_slot + n_games x P beyond the engine's slots, a workspace that is NULL, misaligned or short, sims of 0,
 *   max_moves outside 1..127, position arrays given in part, collect / stats / read before start. */
typedef struct raz_analysis raz_analysis;
#define RAZ_ANALYSIS_TOP 8
#define RAZ_ANALYSIS_MAX_MOVES 127
#define RAZ_ANALYSIS_ENTRY_PASS (-1)
#define RAZ_ANALYSIS_ENTRY_END (-2)
#define RAZ_ANALYSIS_POS_NONE 0         /* beyond the list, or beyond the end of the game */
#define RAZ_ANALYSIS_POS_SEARCH 1       /* its slot was armed */
#define RAZ_ANALYSIS_POS_PASS_ENTRY 2   /* the entry from here is a pass entry: the position is the one after it too, searched there */
#define RAZ_ANALYSIS_POS_OVER 3         /* the game ended here, by the rules or by an illegal move */
#define RAZ_ANALYSIS_END_LIST 0         /* the list ended with the game running */
#define RAZ_ANALYSIS_END_RULES 1        /* neither side could move */
#define RAZ_ANALYSIS_END_ILLEGAL 2      /* a move that flips nothing: the mover lost (reversi_env.py:90-93) */
#define RAZ_ANALYSIS_EVAL_NONE 0        /* not a SEARCH position */
#define RAZ_ANALYSIS_EVAL_PENDING 1
#define RAZ_ANALYSIS_EVAL_SEARCHED 2
#define RAZ_ANALYSIS_EVAL_SOLVED 3
#define RAZ_ANALYSIS_EVAL_ERROR 4
#define RAZ_ANALYSIS_ERR_SLOT 0x100u       /* a slot finished outside the one-move protocol (phase done, or idle without exactly one ply) */
#define RAZ_ANALYSIS_ERR_BAD_CODE 0x400u   /* a list entry outside -2..63 */
typedef struct {
    uint64_t black, white;       /* the board, absolute colours */
    uint8_t player;              /* side to move: 1 black / 2 white */
    uint8_t state;               /* RAZ_ANALYSIS_POS_* */
    uint8_t moves_made;          /* j */
    int8_t played;               /* the entry played from here: 0..63, -1 a pass entry, -2 none */
    uint32_t pad;
} raz_analysis_pos;              /* 24 bytes */
typedef struct {
    uint32_t positions;          /* positions written (states other than NONE): 1 + the entries played */
    uint8_t ended;               /* RAZ_ANALYSIS_END_* */
    uint8_t winner;              /* 0 running; 1 black / 2 white / 3 draw */
    uint8_t blacks, whites;      /* disc counts of the last position */
    uint32_t errors;             /* 0 or RAZ_ANALYSIS_ERR_BAD_CODE */
    uint32_t searched;           /* SEARCH positions: slots armed */
} raz_analysis_game;             /* 16 bytes */
typedef struct {
    uint8_t state;               /* RAZ_ANALYSIS_EVAL_* */
    int8_t action;               /* the engine's move: 0..63, -1 = resigned / none */
    uint8_t n_top;               /* entries of top_* in use */
    int8_t played;               /* raz_analysis_pos.played */
    uint32_t sum_n;              /* sum of the root's visit counts */
    double top_q[RAZ_ANALYSIS_TOP];
    uint32_t top_n[RAZ_ANALYSIS_TOP];
    int8_t top_square[RAZ_ANALYSIS_TOP];
    double played_q;
    uint32_t played_n;
    uint32_t flags;              /* state ERROR: the slot's engine error flags | RAZ_ANALYSIS_ERR_SLOT */
} raz_analysis_eval;             /* 128 bytes */
typedef struct {
    uint32_t games;              /* games replayed by raz_analysis_start */
    uint32_t positions;          /* positions written */
    uint32_t armed;              /* SEARCH positions */
    uint32_t pending;            /* of those, not yet collected */
    uint32_t searched, solved, failed;   /* collected, by eval state */
    uint32_t error;              /* 0, or engine error flags of a slot (1 pool, 2 table, 4 records, 8 path) | RAZ_ANALYSIS_ERR_* */
} raz_analysis_stats;            /* 32 bytes */
size_t raz_analysis_workspace_bytes(uint32_t n_games, uint32_t max_moves);
int raz_analysis_create(raz_engine* engine, uint32_t first_slot, void* d_workspace, size_t workspace_bytes, uint32_t n_games,
                        uint32_t max_moves, raz_analysis** out);
void raz_analysis_destroy(raz_analysis* a);
int raz_analysis_start(raz_analysis* a, const uint64_t* d_black, const uint64_t* d_white, const uint8_t* d_player,
                       const int8_t* d_moves, uint32_t sims, raz_stream_t stream);
int raz_analysis_collect(raz_analysis* a, raz_stream_t stream);
int raz_analysis_stats_sync(raz_analysis* a, raz_analysis_stats* out, raz_stream_t stream);
int raz_analysis_read(raz_analysis* a, raz_analysis_game* games, raz_analysis_pos* positions, raz_analysis_eval* evals,
                      raz_stream_t stream);

/* ---- a league of up to 16 models on the device (csrc/raz_league.h) ---------------------------------------------------
 * raz_match_* with the pairing of every game spelled out.  A league couples n_models (2..RAZ_LEAGUE_MAX_MODELS) STARTED engines, one
 * per model, which may differ in n_games, and plays n_games games at once: game g names its two models and, for each, the slot of that
 * model's engine that is its player in the game (raz_league_pairing), with the tree, random streams and one-move semantics
 * raz_engine_set_position gives that slot.  The caller steps the engines.  The league lives in a caller-provided device workspace
 * (raz_league_workspace_bytes(n_models, slots_per_model, n_games) bytes, slots_per_model[m] = engine m's n_games; 256-byte aligned,
 * owned by the caller, as are the engines, for the lifetime of the handle; 0 is returned, with a message, for n_models outside 2..16,
 * n_games == 0 or a NULL array):
 *   raz_league_stats and the models' simulations a move u32[16] | raz_engine_dev [n_models] (the engines' descriptors: a table in
 *   HBM, not kernel arguments) |
 *   raz_league_pairing [n_games] | raz_league_game [n_games] | raz_league_ply [n_games][64] | one u32 claim word per slot of every
 *   engine | root visit counts u32 [n_games][64][64], each section rounded up to 256 bytes.
 * raz_league_start: memsets of the counters, games, log headers and claim words, the descriptor table written on `stream`, and two
 *   launches of one thread per game.  The first copies d_pairings[g] into the workspace (the caller's array need not outlive the call's
 *   work on `stream`) and, where the pairing is SOUND - both model indices < n_models and different, both slots < their engine's
 *   n_games - does atomicMin(claim[model][slot], g) on both slots.  The second starts game g where its pairing is sound AND both claim
 *   words hold g: the lowest game index wins a contested slot, whatever the launch order.  A game not started gets
 *   RAZ_LEAGUE_GAME_NOT_STARTED and searching 0, is never counted live, and RAZ_LEAGUE_ERR_PAIRING goes into the error word.  Every
 *   other game starts as raz_match_start starts one: (d_black[g], d_white[g], d_player[g]) - nullable, all or none: NULL = the initial
 *   position, black to move; playable positions are the caller's guarantee - with the side to move armed in its model's engine at its
 *   slot: the mover's own discs as "black", player 1, sims_per_model[model] (a HOST array of n_models entries) simulations, one move.
 *   Slots no started game names are not touched.
 * raz_league_turn: the engines' present descriptors are compared with the uploaded copies (host memcmp) and uploaded again, ordered on
 *   `stream`, where they differ; then one launch over all games under raz_match_turn's rule, with (model, slot) read from the game's
 *   pairing and the engine from the table.  An engine error flag, phase done, an idle slot without exactly one ply, or a 65th ply ends
 *   the game and ORs into the error word: a league never spins.
 * raz_league_stats_sync: the counters (synchronises `stream`).  raz_league_read: the games, the pairings as kept, the log and the root
 *   visit counts to host arrays of n_games, n_games, n_games x 64 and n_games x 64 x 64 entries (any may be NULL; synchronises).
 * RAZ_EINVAL / RAZ_ESTATE with a message and NO launch: a NULL argument, n_models outside 2..16, n_games == 0, the same engine twice,
 *   an engine not started, a workspace that is NULL, misaligned or short, a sims entry of 0, position arrays given in part or
 *   misaligned, turn / read / stats before start. */
typedef struct raz_league raz_league;
#define RAZ_LEAGUE_MAX_MODELS 16
#define RAZ_LEAGUE_MAX_PLIES RAZ_MATCH_MAX_PLIES
typedef struct {
    uint8_t black_model, white_model;   /* model indices: which engine plays black / white */
    uint16_t pad0;
    uint32_t black_slot, white_slot;    /* the slot of black_model's / white_model's engine that plays this game */
    uint32_t pad1;
} raz_league_pairing;            /* 16 bytes */
typedef struct {
    uint64_t black, white;       /* the real board, absolute colours */
    uint8_t player;              /* side to move: 1 black / 2 white */
    uint8_t black_model, white_model;
    uint8_t searching;           /* whose slot is searching: 0 nobody (ended, or not started), 1 black's model's, 2 white's model's */
    uint8_t winner;              /* 0 running; 1 black / 2 white / 3 draw */
    uint8_t blacks, whites;      /* disc counts when the game ended */
    uint8_t n_plies;             /* entries of the game's log */
    uint8_t flags;               /* 0x10 ended by an illegal move, 0x20 by a resignation (as raz_env_step) | RAZ_LEAGUE_GAME_NOT_STARTED */
    uint8_t pad8[3];
    uint32_t pad;
} raz_league_game;               /* 32 bytes */
#define RAZ_LEAGUE_GAME_NOT_STARTED 0x40u   /* the pairing was unsound, or a lower game index holds one of its slots */
typedef struct {
    uint8_t who;                 /* the model index that moved */
    int8_t action;               /* 0..63, -1 = resigned */
    uint8_t turn, pad;
} raz_league_ply;                /* 4 bytes */
typedef struct {
    uint32_t live;               /* games still running */
    uint32_t plies;              /* plies handed off since raz_league_start */
    uint32_t error;              /* 0, or engine error flags of a slot (1 pool, 2 table, 4 records, 8 path) | RAZ_LEAGUE_ERR_* */
    uint32_t n_models;
    uint32_t searching[RAZ_LEAGUE_MAX_MODELS];   /* slots searching per model */
    uint32_t pad[12];
} raz_league_stats;              /* 128 bytes */
#define RAZ_LEAGUE_ERR_SLOT 0x100u       /* a searching slot finished outside the one-move protocol (phase done, or idle without exactly one ply) */
#define RAZ_LEAGUE_ERR_LOG_FULL 0x200u   /* a game's 65th ply */
#define RAZ_LEAGUE_ERR_PAIRING 0x800u    /* raz_league_start left a game out (RAZ_LEAGUE_GAME_NOT_STARTED) */
size_t raz_league_workspace_bytes(uint32_t n_models, const uint32_t* slots_per_model, uint32_t n_games);
int raz_league_create(raz_engine* const* engines, uint32_t n_models, void* d_workspace, size_t workspace_bytes, uint32_t n_games,
                      raz_league** out);
void raz_league_destroy(raz_league* l);
int raz_league_start(raz_league* l, const raz_league_pairing* d_pairings, const uint64_t* d_black, const uint64_t* d_white,
                     const uint8_t* d_player, const uint32_t* sims_per_model, int enable_resign, raz_stream_t stream);
int raz_league_turn(raz_league* l, raz_stream_t stream);
int raz_league_stats_sync(raz_league* l, raz_league_stats* out, raz_stream_t stream);
int raz_league_read(raz_league* l, raz_league_game* games, raz_league_pairing* pairings, raz_league_ply* log, uint32_t* log_root_n,
                    raz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RAZ_H */
