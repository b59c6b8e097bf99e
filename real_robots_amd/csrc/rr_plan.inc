// rr_plan.inc -- the schedule of one step as a decision: plan_step() maps the batch's shape, the handle's settings and ONE reading of
// the two lagged list lengths to a StepPlan; rr_step (rr_host.inc) computes it once per step and step_split / step_split_timed /
// step_single / launch_render / launch_solve_class carry it out without reading a count or a threshold again.  Pure integer logic:
// no HIP type, no rr_env, nothing beyond <algorithm> -- tests/test_step_plan.py compiles it alone and compares every decision with a
// restatement over the thresholds' neighbourhoods.  No plan may change a result, only where and in which shape the work is launched
// (every placement is forced and compared bitwise against the in-line step, tests/test_gpu_round4.py).
//
// The placements (DESIGN.md 5.2):
//   1. split, a handful of very heavy envs (the benchmark's early window): look-ahead behind the very heavy envs' solve (la_on_vh);
//      1'. with a LONG heavy list (late window) the very heavy envs' render moves to the tail of the main stream (vh_render_on_main);
//   2. split, hundreds of very heavy envs AND a long heavy list (macro actions): kinematics + collision pass of the look-ahead on the
//      heavy stream, its dynamics half on the very heavy one (la_side);
//   3. mostly heavy envs, or a step without camera: one solve launch for everybody, look-ahead beside the render (PATH_SINGLE);
//   3b. a step without camera of a large batch with a long very heavy list: the classes side by side, the very heavy envs a wave each
//      (SOLVE_SIDE_BY_SIDE);
//   4. a handful of envs (the gym facade): one chain on the main stream, the mirror in front of the look-ahead (small_n);
//   5. the reference: everything in line (split_heavy / lookahead off; the timing leg of bench.py runs placement 1's launches one
//      after the other under their timers, PATH_SPLIT_TIMED).
#include <algorithm>

// ---- the thresholds the plan reads (defined here and nowhere else) -----------------------------------------------------------------
#define COOP_MAX 256        // (1024 measured on the macro workload, 388 very heavy envs: no gain) lists up to this long (lagged host count) are solved one env per wave (coop row build); longer ones four to a wave
#define COOP_MAX_VH 512     // the same for the very heavy list (StepPlan::coop_vh_*)
#define RENDER_LIST_WGS 768      // workgroups of the heavy lists' one-launch render (k_render_list in rr_render.inc; two resident per CU: set-up, visibility and shading in one body need 128 VGPRs -- capped at 80 it spilled); a heavy list of more (env, tile) items is "long" (h_long)
#define COOP_ALL_MAX 1024   // up to this many envs a step that solves all envs in one launch gives every env its own wave (Settings::coop_all off: four to a wave)
#define SMALL_N_MAX 64      // up to this many envs a step without the three-stream split runs as one chain on the main stream
#define LA_VH_MAX 64         // look-ahead behind the very heavy envs' solve while their (lagged) number is at most this
#define NORENDER_SPLIT_VH_MIN 64   // a step without camera runs its classes side by side from this many (lagged) very heavy envs on
// (a heavy list of more than a third of the batch -- macro actions: 1 500 .. 2 000 of 4 096 envs -- is rasterised by the grid kernel
// over all (env, tile) workgroups, those of other classes leaving at once: four workgroups per CU at 64 VGPRs instead of the
// list walker's three at 79; macro workload 1.130 -> 1.101 ms.  A list of 660 envs -- the late window -- is better off with the
// walker: 0.679 against 0.711 ms)
// The threshold was a quarter of the batch until round 6; the off-bench schedule test (tests/test_gpu_round6.py: 1 230 heavy envs
// of 4 096 pressing the gripper on the table) measured the walker 3.6 % ahead there, the macro workload (1 486 .. 1 969 heavy
// envs) the grid 2.5 % ahead of a threshold of 0.4: a third of the batch lies between the two measured sides.
#define GRID_RASTER_DENOM 3

// The lagged host copies of the heavy (h) / very heavy (vh) list lengths as rr_step read them, once, for this step.  known == false:
// there is nothing to read (the pinned word could not be allocated); every predicate then falls back on its own side -- the
// list-walking render and the coop solves assume a long list (N), the others an empty one (0).
struct PlanCounts { int h, vh; bool known; };
struct PlanIn {
    int N, ntiles, render_mode;     // envs, raster tiles per env, rr_step's render_mode (0: a step without camera)
    bool timing;                    // the timing leg: everything on the main stream under its timers
    bool split_heavy, lookahead, coop_all; int split_max_pct;     // Settings
    PlanCounts counts;
};

enum PlanPath { PATH_SPLIT, PATH_SPLIT_TIMED, PATH_SINGLE };                    // step_split / step_split_timed / step_single
enum HeavyRender { RENDER_WALKER, RENDER_RASTER_LIST, RENDER_GRID };             // k_render_list | k_raster_list + k_shade | grid k_raster + k_shade
enum SingleSolve { SOLVE_CHAIN_N1, SOLVE_SIDE_BY_SIDE, SOLVE_WAVE_PER_ENV, SOLVE_PACKED };
struct StepPlan {
    PlanPath path;
    bool mostly_heavy;              // more than split_max_pct of the envs are heavy -- macro actions, every gripper pushing: nothing to gain from the split
    bool h_long;                    // the heavy list is too long for one list-walking render launch
    HeavyRender heavy_render;       // the render of the heavy list (the very heavy one is always walked by one launch)
    bool coop_h;                    // heavy solve one env per wave (else four to a wave)
    bool coop_vh_beside, coop_vh_alone;    // the same for the very heavy solve, beside a visibility pass / in a step without camera
    // PATH_SPLIT only
    bool la_on_vh, la_side;         // look-ahead behind the very heavy envs' solve (placement 1), held behind the light envs' visibility pass by an event / split over the two side streams (2)
    bool vh_render_on_main, vh_render_on_aux;      // the very heavy envs' render at the main stream's tail (1') / behind the heavy envs' (1); neither: on their own stream (2, no look-ahead)
    // PATH_SINGLE only
    bool small_n;                   // placement 4
    SingleSolve single_solve;       // ONE env class by class | 3b | one launch, a wave per env | one launch, four envs to a wave
    bool la_beside;                 // the state part of the next step on the side stream beside the render of this one
};

static inline StepPlan plan_step(const PlanIn &in) {
    const int N = in.N;
    const PlanCounts &c = in.counts;
    const int h0 = c.known ? c.h : 0, vh0 = c.known ? c.vh : 0;      // the readings with the fallback of an empty list ...
    const int hN = c.known ? c.h : N, vhN = c.known ? c.vh : N;      // ... and of a long one
    const bool ahead = in.lookahead;            // the step ends with the state part of the next one
    StepPlan p;
    // (the number of heavy envs of a recent step, written to pinned host memory by the solve kernel without anybody waiting for it)
    p.mostly_heavy = (long long)h0 * 100 > (long long)N * in.split_max_pct;
    // (a step without camera runs all envs in one launch: its classes side by side measured 0.525 instead of 0.452 ms on config 2;
    // ONE env -- the gym facade -- renders in its chain on the main stream too: the split has nothing to overlap there)
    const bool split = in.render_mode && in.split_heavy && !p.mostly_heavy && !(N == 1 && !in.timing);
    p.path = !split ? PATH_SINGLE : (in.timing ? PATH_SPLIT_TIMED : PATH_SPLIT);

    // (a long heavy list is rendered by three launches, the longest chain of the step: the very heavy envs' render then goes to the
    // tail of the main stream, which is done with the shading by then)
    p.h_long = (long long)h0 * in.ntiles > RENDER_LIST_WGS;
    // the heavy envs, a few (at most one item per workgroup): one list-walking launch for set-up, visibility and shading -- the tail
    // of the step's longest chain; many: the three kernels (the fused one needs 128 VGPRs: two workgroups per CU, which a long list
    // pays for), the visibility pass by the list walker or, from a third of the batch on, by the grid kernel
    p.heavy_render = (long long)hN * in.ntiles <= RENDER_LIST_WGS ? RENDER_WALKER
                   : ((long long)h0 * GRID_RASTER_DENOM > (long long)N ? RENDER_GRID : RENDER_RASTER_LIST);

    // A list of at most COOP_MAX entries is solved in the coop form: one env per wave, four waves per workgroup with one LDS region
    // each (N waves: whatever the list's actual length, every entry has its wave; the others exit at once); a longer one four envs
    // to a wave.
    // (the very heavy list in the coop form up to COOP_MAX_VH entries: its solve is the step's longest chain -- round 6's off-bench
    // schedule check, 410 arms crushed on the table: 0.672 packed, 0.632 ms one env per wave; a long HEAVY list stays packed from
    // COOP_MAX on: 700 waves with an LDS region each crowd the visibility pass out, NOTEBOOK.md B)
    // -- unless the heavy list is long too (macro actions: 1 500+ heavy envs, packed, beside 380 very heavy ones: 3.82 -> 3.76 M in the coop form)
    p.coop_h = hN <= COOP_MAX;
    p.coop_vh_beside = vhN <= (p.h_long ? COOP_MAX : COOP_MAX_VH);
    // (a step without camera -- no visibility pass for the one-env-per-wave form's LDS regions to crowd out)
    p.coop_vh_alone = vhN <= COOP_MAX_VH;

    // placement 1 (else 2).  Placement 2 -- the look-ahead split over the two side streams -- was tuned on the macro workload (hundreds
    // of very heavy envs AND 1 500+ heavy ones); with many very heavy envs but a short heavy list (round 6's off-bench schedule
    // check: 410 arms crushed on the table, no other heavy env) placement 1 is 7.8 % faster: both lists must be long for 2.
    p.la_on_vh = ahead && (vh0 <= LA_VH_MAX || !p.h_long);
    p.la_side = ahead && !p.la_on_vh;
    p.vh_render_on_main = p.la_on_vh && p.h_long;
    p.vh_render_on_aux = p.la_on_vh && !p.vh_render_on_main;
    // (placement 1's look-ahead is HELD behind the light envs' visibility pass by an event, step_split: k_prep_ab16 -- 128-thread
    // workgroups of <= 128 VGPRs -- gets onto the machine at once, and the collision pass behind it, 39 KB of LDS per workgroup,
    // would then run beside the visibility pass and crowd it out.  A preparation whose waves each needed a whole free SIMD, rounds
    // 1-5, sat in its queue until the visibility pass' grid was exhausted and kept the collision pass out of its way unasked.)

    p.small_n = N <= SMALL_N_MAX && in.split_heavy && !in.timing;
    // Placement 3b: a step without camera whose very heavy list is long (macro actions without the retina: 368 of 4 096 envs).  In the
    // one launch for everybody those envs are solved four to a wave, sixteen lanes building the rows of an env at the contact cap; side
    // by side on the three streams they get a wave each -- 0.765 -> 0.711 ms per step on the macro workload.  With a handful of
    // very heavy envs (the headline's population) the one launch is ahead, 0.491 against 0.516 ms: the forks and joins cost more
    // than the few long chains gain.
    const bool side_by_side = !in.render_mode && N > COOP_ALL_MAX && in.split_heavy && !in.timing && vh0 >= NORENDER_SPLIT_VH_MIN;
    p.single_solve = p.small_n && N == 1 ? SOLVE_CHAIN_N1
                   : (side_by_side ? SOLVE_SIDE_BY_SIDE
                   : (in.coop_all && N <= COOP_ALL_MAX && in.split_heavy ? SOLVE_WAVE_PER_ENV : SOLVE_PACKED));
    // (with a camera the state part of the next step runs on the side stream beside the render of this one; the timing leg has no
    // side streams)
    p.la_beside = ahead && in.render_mode && !in.timing && !p.small_n;
    return p;
}
