// raz_engine_fused.hip — tree + net in ONE kernel for narrow nets: k_tree_net and k_tree_par_net, built on the bodies they share with
// k_tree / k_tree_par (raz_engine_core.h: load_game, tree_steps, load_game_and_slots, par_round, run_controller).
//
// With the F == 16 net (mini.yml) a step of the classic pipeline is two latency-bound launches per slice - k_tree (25 us) and
// k_net_mfma (one wave per position, 13-25 us) - handing leaves and answers over through HBM, and its rate is set by that chain's
// latency and by how many launches per second one host thread and the hardware queues sustain (more than three
// slices or hipGraph replay made it slower).  Here the game's wave evaluates its own leaf: the descent ends with the position
// in registers, raz_net16_forward_in_wave (raz_net_wave.h: matrix-core trunk in one LDS plane buffer of this wave, heads as
// k_net_mfma) returns the policy row and the value into the registers backup_leaf reads, and the loop goes on with the next
// simulation - `iters` of them per launch, the control block and the path staying in registers throughout.  No leaf exchange, no
// second kernel, no slices; one launch per `iters` simulation steps of the whole batch.  4 waves per SIMD (128 VGPRs, 9.7 KB of
// LDS per wave): 4096 games are resident at once.  Measured resources (-Rpass-analysis=kernel-resource-usage): k_tree_net<false>
// spills 31 VGPRs (128 B of scratch per lane) around the in-wave net call - most of the kernel's counter traffic
// (profiles/r4_pmc/config1_fused_*), and cheaper than not spilling (below) - k_tree_par_net<false> none; the SOLVER forms are at 4 waves per SIMD too since round 5 (the end-game search
// itself runs in the solver pool, raz_solver_pool.h: these kernels only post positions and solve <= 4 empties in place; a game whose
// request is in flight leaves the launch, and the pool gets its round after every <= 8 fused steps).  Every game performs exactly the
// operations it performs under k_tree + k_net_mfma, in the same order: results are bit-identical (tests/test_engine_fused_emu.py
// on the wave emulator, tests/test_engine_gpu.py, tests/test_zz_fused_gpu.py).  raz_engine_config.reserved bit 4, without the
// evaluation cache; the worker's default for 16-filter nets when the solver is off (105 M against 77 M sims/s on BASELINE
// configs[1]).  At the end of a launch the last leaf's answer is parked in nn_policy / nn_value exactly where k_net_mfma would
// have put it, so the two forms can even alternate.
#include <hip/hip_runtime.h>
#include "raz_engine_core.h"
#include "raz_net_wave.h"   // raz_net16_forward_in_wave

#ifndef RAZ_FUSED_ITERS
#define RAZ_FUSED_ITERS 256   // most simulation steps per launch (32 -> 256: +0.9 % on configs[1], profiles/r5/fused_kernel_ab.json)
#endif

namespace {

// -DRAZ_FUSED_PROF (measurement builds only): shader-clock ticks of a step's phases of k_tree_net into the engine's phase profile
// (engine.phase_profile(): 0 backup, 1 controller, 2 select, 5 the in-wave forward; the engine created with phase_profile=True)
#ifdef RAZ_FUSED_PROF
constexpr int kFusedProf = kProfFused;
#else
constexpr int kFusedProf = kProfNone;
#endif

template <bool SOLVER>
__global__ __launch_bounds__(64) RAZ_TREE_WAVES(SOLVER) void k_tree_net(raz_engine_dev E, uint32_t g0, uint32_t count,
                                                                                          uint32_t iters, const float* __restrict__ net_w,
                                                                                          int net_R, int net_V) {
    if (blockIdx.x >= count) return;
    // LDS of the wave: the net's plane buffer, then ONE scratch area shared in time by the net's heads (during a forward), the
    // reduction scratch of backup_leaf and the solver's frames (between forwards; both are initialised by their users on every
    // call) - 9.7 KB in all, so that 16 waves fit a CU's 160 KB whatever the allocation granule
    extern __shared__ __attribute__((aligned(16))) float netbuf[];
    float* lds64 = netbuf + 16 * PS;
    SolverLDS* slds_p = SOLVER ? (SolverLDS*)(netbuf + 16 * PS + 64) : nullptr;
    const uint32_t g = g0 + blockIdx.x;
    const int lane = threadIdx.x;
    if (g >= E.B) return;
    if (SOLVER && solve_in_flight(E, g)) return;   // the request is still with the solver pool: nothing to do in this launch
    uint32_t* gw = (uint32_t*)(E.game + g);
    Regs R;
    if (!load_game<kProfNone>(E, R, gw, g, lane)) return;
    raz_net16_zero_planes(netbuf, lane);
    tree_steps<SOLVER, kFusedProf>(E, R, g, lane, lds64, slds_p, iters, [&](unsigned long long& t_prof) {
        // what select_leaf handed to the leaf exchange (nn_own / nn_enemy), recomputed from the control block: the
        // leaf's position under the D4 transform drawn for it, from the side to move's view (player.py:299-309)
        const uint32_t sym = G32(R, GW(leaf_sym));
        const raz_bb lb = G64(R, GW(leaf_b)), lw = G64(R, GW(leaf_w));
        const raz_bb tb = bb_d4_apply(lb, (int)(sym >> 2) & 1, (int)(sym & 3)), tw = bb_d4_apply(lw, (int)(sym >> 2) & 1, (int)(sym & 3));
        const bool black_to_move = G32(R, GW(leaf_np)) == 1u;
        raz_net16_forward_in_wave(net_w, net_R, net_V, black_to_move ? tb : tw, black_to_move ? tw : tb, netbuf, lane, R.pol_raw, R.val);
        R.nn = 0u;
        if (kFusedProf) prof_add(E, g, 5, t_prof, lane);
    });
    gw[lane] = R.cw;
    if (R.path_dirty) path_store(E, R, (size_t)g, lane);
    // the answer for a leaf that is still to be backed up waits where the net kernel would have left it
    E.nn_policy[(size_t)g * 64 + lane] = R.pol_raw;
    if (lane == 0) {
        E.nn_value[g] = R.val;
        E.nn_active[g] = 0;
    }
}

// The same for parallel_search_num > 1: k_tree_par's round (par_round) followed by the evaluation of the round's queued leaves by the
// game's own wave, one after the other, `iters` times per launch.  One iteration is exactly one launch of k_tree_par + the net batch of
// the classic pipeline - including a fill that ran out of its per-launch budget and goes on after the evaluation without a B in between -
// so the raz-sched-v1 schedule, and with it every record, is unchanged.  The slot states stay in registers across iterations; the
// leaves' positions and answers still travel through the leaf-exchange rows (written and read by this wave only).
template <bool SOLVER>
__global__ __launch_bounds__(64) RAZ_TREE_WAVES(SOLVER) void k_tree_par_net(raz_engine_dev E, uint32_t g0, uint32_t count,
                                                                                              uint32_t iters, const float* __restrict__ net_w,
                                                                                              int net_R, int net_V) {
    if (blockIdx.x >= count) return;
    // LDS of the wave: as k_tree_net's
    extern __shared__ __attribute__((aligned(16))) float netbuf[];
    float* lds64 = netbuf + 16 * PS;
    SolverLDS* slds_p = SOLVER ? (SolverLDS*)(netbuf + 16 * PS + 64) : nullptr;
    const uint32_t g = g0 + blockIdx.x;
    const int lane = threadIdx.x;
    if (g >= E.B) return;
    if (SOLVER && solve_in_flight(E, g)) return;   // the request is still with the solver pool: nothing to do in this launch
    const uint32_t K = E.K;
    uint32_t* gw = (uint32_t*)(E.game + g);
    Regs R;
    Slots T;
    if (!load_game_and_slots<kProfNone>(E, R, T, gw, g, K, lane)) return;
    raz_net16_zero_planes(netbuf, lane);
    const raz_engine_dev& E0 = E;
    for (uint32_t it = 0; it < iters; ++it) {
        const raz_engine_dev& E = fresh_descriptor(E0);
        {
            const uint32_t phase = G32(R, GW(phase));
            if (phase == RAZ_PHASE_DONE || phase == RAZ_PHASE_IDLE || G32(R, GW(error))) break;
        }
        const uint32_t nnmask = par_round<SOLVER, kProfNone, true>(E, R, T, g, K, lane, lds64, slds_p);
        // ---- the net batch of this iteration: the leaves queued above, evaluated by this wave (their answers go where the net
        // kernel would have put them; the B stage of the next round picks them up with slot_load)
        wave_sync();
        for (uint32_t m = nnmask; m; m &= m - 1) {
            const int ln = fresh_lane(lane);
            const uint32_t jj = (uint32_t)__ffs((int)m) - 1u;
            const size_t gi = (size_t)g * K + jj;
            const raz_bb own = uni((raz_bb)E.nn_own[gi]), enemy = uni((raz_bb)E.nn_enemy[gi]);
            float pol, val;
            raz_net16_forward_in_wave(net_w, net_R, net_V, own, enemy, netbuf, ln, pol, val);
            E.nn_policy[gi * 64 + ln] = pol;
            if (ln == 0) E.nn_value[gi] = val;
        }
        wave_sync();
        if (SOLVER && R.solve_pending) break;   // a solve (the root's, or one inside a simulation) waits for the next launch's budget
    }
    write_back_game_and_slots<SOLVER>(E, R, T, gw, g, K, fresh_lane(lane), 0u);
}

}  // namespace

// `n_steps` simulation steps of the whole batch in ceil(n_steps / 32) launches on stream s (raz_engine_step, reserved bit 4)
int raz_launch_tree_net(const raz_engine_dev& d, bool solver, uint32_t n_steps, const float* W, int R, int V, hipStream_t s) {
    constexpr uint32_t kFusedIters = RAZ_FUSED_ITERS;
    // behind the plane buffer: the heads' scratch of a forward, shared in time with backup_leaf's 64 floats and - solver forms only - the
    // scalar end-game search's frames (704 B); 16 waves per CU x 9.7 KB either way
    const int between = 64 + (solver ? (int)(sizeof(SolverLDS) / sizeof(float)) : 0);
    const int head = (int)heads_lds_floats(V) > between ? (int)heads_lds_floats(V) : between;
    const size_t shm = ((size_t)16 * PS + head) * sizeof(float);
    int rc = RAZ_OK;
    while (n_steps && rc == RAZ_OK) {
        const uint32_t it = n_steps < kFusedIters ? n_steps : kFusedIters;
        if (d.par && solver)
            hipLaunchKernelGGL(k_tree_par_net<true>, dim3(d.B), dim3(64), shm, s, d, 0u, d.B, it, W, R, V);
        else if (d.par)
            hipLaunchKernelGGL(k_tree_par_net<false>, dim3(d.B), dim3(64), shm, s, d, 0u, d.B, it, W, R, V);
        else if (solver)
            hipLaunchKernelGGL(k_tree_net<true>, dim3(d.B), dim3(64), shm, s, d, 0u, d.B, it, W, R, V);
        else
            hipLaunchKernelGGL(k_tree_net<false>, dim3(d.B), dim3(64), shm, s, d, 0u, d.B, it, W, R, V);
        rc = raz_check_launch("raz_engine_step: k_tree_net");
        n_steps -= it;
    }
    return rc;
}
