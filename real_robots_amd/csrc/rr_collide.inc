// rr_collide.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_collide: the collision pass (contact lists, warm-start matching, env classes)
// ---------------------------------------------------------------------------------------------- k_collide
struct Xf { m3 R; v3 p; };

// World transform of the owner of shape s.  All loads are unconditional and from always-valid addresses (the values are
// selected afterwards): with loads under the owner-type branches the compiler merges the branches into a select of base
// pointers whose value is undefined on the static path and may still issue the load -- a fault at a garbage address.
__device__ __forceinline__ Xf load_xf(const ShapeData *S, int s, const float *scratch, int env) {
    Xf X;
    const int ot = S->otype[s];
    const int oi = ot == 0 ? 0 : S->oidx[s];
    const int rslot = (ot == 1 ? S_BR : S_OR) + 9 * oi;
    float r[9];
    r[0] = SCR(rslot); r[1] = SCR(rslot + 1); r[2] = SCR(rslot + 2); r[3] = SCR(rslot + 3); r[4] = SCR(rslot + 4);
    r[5] = SCR(rslot + 5); r[6] = SCR(rslot + 6); r[7] = SCR(rslot + 7); r[8] = SCR(rslot + 8);
    const int ob = ot == 2 ? oi : 0, bb = ot == 1 ? oi : 0;
    const float pbx = SCR(S_BP + 3 * bb), pby = SCR(S_BP + 3 * bb + 1), pbz = SCR(S_BP + 3 * bb + 2);
    const float pox = SCR(S_OP + 3 * ob), poy = SCR(S_OP + 3 * ob + 1), poz = SCR(S_OP + 3 * ob + 2);      // (the pose that counts: prep_body<1>)
    const bool st = ot == 0, body = ot == 1;
    X.R.m[0] = st ? 1.0f : r[0]; X.R.m[1] = st ? 0.0f : r[1]; X.R.m[2] = st ? 0.0f : r[2];
    X.R.m[3] = st ? 0.0f : r[3]; X.R.m[4] = st ? 1.0f : r[4]; X.R.m[5] = st ? 0.0f : r[5];
    X.R.m[6] = st ? 0.0f : r[6]; X.R.m[7] = st ? 0.0f : r[7]; X.R.m[8] = st ? 1.0f : r[8];
    X.p = mk(st ? 0.0f : (body ? pbx : pox), st ? 0.0f : (body ? pby : poy), st ? 0.0f : (body ? pbz : poz));
    return X;
}

#ifdef RR_RASTER_STATS
// development build only: cycle stamps of kernel phases (lane 0 of every block), see scratch/sprof.py
__device__ unsigned long long g_sprof[16];
#define SPROF(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); sp_acc[i] += (unsigned)(now_ - sp_t0); sp_t0 = now_; } while (0)   /* cheap phase clock: s_memtime into per-wave accumulators, flushed once (SBLK_END); RR_ABLATE = block << 16 | 0x4000: one block only */
#define SPROF_INIT unsigned long long sp_t0 = __builtin_readcyclecounter(); unsigned sp_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define SPROF_FLUSH do { if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) == ((!GEN && LIGHT_OW_THREADS == 384) ? 1 : 0) && (!(P.ablate & 0x4000) || (int)blockIdx.x == (P.ablate >> 16))) { _Pragma("unroll") for (int i_ = 0; i_ < 12; i_++) atomicAdd(&g_sprof[i_], (unsigned long long)sp_acc[i_]); } } while (0)
// per solver workgroup: {total cycles, cycles up to the end of the row build, cycles of the PGS loop, -, then per env
// nc | generic contacts << 8 | leading object-vs-static contacts << 16 | last F-list length << 24}
__device__ unsigned g_sblk[4096 * 8];
#define SBLK_BEGIN const unsigned long long sb_t0 = __builtin_readcyclecounter(); unsigned long long sb_t1 = sb_t0, sb_t2 = sb_t0;
#define SBLK_MARK(v) v = __builtin_readcyclecounter();
#define SBLK_END(ncv, gv, osv, nfv) do { if (unit < 4096) { if (l == 0) g_sblk[unit * 8 + 4 + (grp & 3)] = (unsigned)(ncv) | ((unsigned)(gv) << 8) | ((unsigned)(osv) << 16) | ((unsigned)(nfv) << 24); \
    if ((threadIdx.x & 63) == 0) { g_sblk[unit * 8] = (unsigned)(__builtin_readcyclecounter() - sb_t0); g_sblk[unit * 8 + 1] = (unsigned)(sb_t1 - sb_t0); g_sblk[unit * 8 + 2] = (unsigned)(sb_t2 - sb_t1); } } } while (0)
extern "C" int rr_debug_solver_blocks(unsigned *out, int nblocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sblk), sizeof(unsigned) * 8 * (size_t)nblocks) == hipSuccess ? 0 : -1;
}
extern "C" int rr_debug_solver_prof(unsigned long long *out16, int reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sprof), sizeof(g_sprof)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sprof), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#else
#define SPROF(i)
#define SPROF_INIT
#define SPROF_FLUSH
#define SBLK_BEGIN
#define SBLK_MARK(v)
#define SBLK_END(ncv, gv, osv, nfv)
#endif

// ---- collision: one wavefront per env ------------------------------------------------------------------------------
// Every collision shape is the convex hull of its OBJ (SURVEY A.1.3) reduced to <= 192 vertices and <= 192 facet planes
// (deviation from the full hull < 1 mm, tests/test_oracle_pins.py).  A contact candidate is a vertex of one shape whose
// largest signed distance to the planes of the other is below the margin; <= 4 points per pair are kept.  A wavefront
// owns an env:
//   1. lanes 0..ns-1 load the transform of "their" shape and its world bounding-sphere centre into LDS (one round trip);
//   2. the pairs are sphere-tested 64 at a time, survivors are collected with ballots;
//   3. every surviving pair is handled by the whole wave, direction 0 (vertices of a against the planes of b) and then
//      direction 1 (b against a):
//        a. exact cull -- the bounding sphere of "mine" beyond one plane of "other" by more than the margin: nothing;
//        b. the planes of "other" are staged in LDS; lane = vertex, 64 at a time: a vertex that is beyond one of the first
//           six planes (the shape's extreme facets along +-x, +-y, +-z) by the margin cannot be a candidate and is dropped
//           (exact: the candidate test is a maximum over ALL planes of the very same values); survivors are compacted,
//           in vertex order, into an LDS list;
//        c. lane = survivor: maximum over all planes (first maximum wins), candidates appended to the pair's list.
//   4. manifold reduction over the candidate list (direction 0 by vertex index, then direction 1 -- the oracle's order):
//      the "first best wins" selections of the oracle's reduce4() are wave reductions with lowest-index tie-breaks.
// The whole kernel is contraction-free (see "contraction-free twins"): results are bit-identical to the oracle's float
// build.  No atomics, no work list: results do not depend on scheduling.
#define COLLIDE_WAVES COLLIDE_WAVES_   // waves per env: the close pairs are dealt out among them (the slowest env sets the kernel's duration)
#define COLLIDE_THREADS (64 * COLLIDE_WAVES)
#define CCHUNK 32         // close pairs whose results are held in LDS at a time (one record writer per kept point; the pair cull leaves 3-4 close pairs per env, 64 cost 2.8 KB more)
#define NPREF 6          // leading planes of every shape used by the prefilter (tools/compile_model.py orders them)
#define CAND_MAX 128     // candidates kept per pair (the oracle applies the same cap)
#define CSHAPES 24       // collision shapes staged in LDS (rr_create checks the model: 22)
#define COLLIDE_WAVES_ 4
#define VH_MAX 1024         // cap of the very heavy list (k_collide)
#ifdef RR_RASTER_STATS
#define CABL(bit) (P.ablate & (bit))      // development build: phase ablations (256 stage only, 512 no pairs, 1024 cull only)
// per-env phase cycles of k_collide (scratch/cprof.py): 0 stage, 1 sphere tests, 2 loads + cull, 3 prefilter, 4 all-plane pass,
// 5 manifold reduction, 6 record write, 7 close pairs
__device__ unsigned g_cprof[8192 * COLLIDE_WAVES_][12];      // 8.. counts: pairs found apart in direction 0 / only in direction 1 / without a candidate / with contacts
extern "C" int rr_debug_collide_prof(unsigned *out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cprof), sizeof(unsigned) * 12 * COLLIDE_WAVES_ * (size_t)n) == hipSuccess ? 0 : -1;   // [n][waves][12]
}
#define CPROF_INIT unsigned cp_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long cp_t0 = __builtin_readcyclecounter();
#define CPROF(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); cp_[i] += (unsigned)(now_ - cp_t0); cp_t0 = now_; } while (0)
#define CPROF_COUNT(i) cp_[i]++
#define CPROF_END do { if (lane == 0 && env < 8192) for (int i_ = 0; i_ < 12; i_++) g_cprof[env * COLLIDE_WAVES_ + wv][i_] = cp_[i_]; } while (0)
#else
#define CABL(bit) false
#define CPROF_INIT
#define CPROF(i)
#define CPROF_COUNT(i)
#define CPROF_END
#endif

// wave-wide "first lane holding the maximum of v among lanes with ok" (returns -1 when no lane is ok or none exceeds
// floor).  The maximum is reduced with DPP row rotations inside each 16-lane row and four v_readlane across the rows
// (an LDS-crossbar butterfly of six dependent ds_bpermute costs ten times as much on a chain this short).
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max(float m) {
    m = fmaxf(m, dpp_mov<0x128>(m));     // row_ror:8
    m = fmaxf(m, dpp_mov<0x124>(m));     // row_ror:4
    m = fmaxf(m, dpp_mov<0x122>(m));     // row_ror:2
    m = fmaxf(m, dpp_mov<0x121>(m));     // row_ror:1  -> every lane holds its row's maximum
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// value of lane src (wave-uniform) in every lane
__device__ __forceinline__ float lane_f(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// number of set bits of m below this lane (v_mbcnt: no lane mask held in registers)
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// exclusive prefix sum over the 64 lanes of a wave (DPP row_shr scan inside each 16-lane row + the row totals)
template <int SHR> __device__ __forceinline__ int dpp_shr0(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x110 + SHR, 0xf, 0xf, true); }
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int &total) {
    int x = v;
    x += dpp_shr0<1>(x); x += dpp_shr0<2>(x); x += dpp_shr0<4>(x); x += dpp_shr0<8>(x);
    const int t0 = __builtin_amdgcn_readlane(x, 15), t1 = __builtin_amdgcn_readlane(x, 31), t2 = __builtin_amdgcn_readlane(x, 47),
              t3 = __builtin_amdgcn_readlane(x, 63);
    const int row = lane >> 4;
    const int off = row == 0 ? 0 : (row == 1 ? t0 : (row == 2 ? t0 + t1 : t0 + t1 + t2));
    total = t0 + t1 + t2 + t3;
    return x + off - v;
}

// the candidate / plane / survivor arrays are private to a wave: LDS traffic is ordered per wave, so a compiler-level fence replaces s_barrier
#define CSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
static_assert(CCHUNK * 4 <= COLLIDE_THREADS && CCHUNK <= 64 && MAXPAIRS < 128 && EMAXC <= 64 && MAXC <= 64, "one record writer per (slot, r); pair ids in 7 bits, edge ids in 6, the contact history staged by one wave");
static_assert(VMAXC % 64 == 0 && FMAXC % 64 == 0 && VMAXC < 256 && FMAXC < 256, "vertex / plane passes of 64, counts packed in bytes");
// (the whole kernel is contraction-free and uses the nc:: helpers: see "contraction-free twins" above)
#pragma clang fp contract(off)
// An edge of a shape in the world frame, and the edge-edge candidate test -- the oracle's edge_edge(), operation for operation.
struct EdgeW { v3 p0, d, n1, n2; };
__device__ __forceinline__ EdgeW edge_world(const float *e, const float *x /* R (9), p (3) */) {
    m3 R;
#pragma unroll
    for (int k = 0; k < 9; k++) R.m[k] = x[k];
    EdgeW E;
    E.p0 = nc::add(nc::mulv(R, mk(e[0], e[1], e[2])), mk(x[9], x[10], x[11]));
    E.d = nc::mulv(R, mk(e[3], e[4], e[5]));
    E.n1 = nc::mulv(R, mk(e[6], e[7], e[8]));
    E.n2 = nc::mulv(R, mk(e[9], e[10], e[11]));
    return E;
}
// true: the closest points of the two edge lines lie strictly inside both segments, the common normal is a face of the
// Minkowski difference and the signed distance along it is inside (-EDGE_DEPTH, margin); cnd = (contact point, distance),
// nrm = the normal B -> A
__device__ __forceinline__ bool edge_pair(const EdgeW &A, const EdgeW &B, float margin, float lo, float4 &cnd, v3 &nrm) {
    const v3 r = nc::sub(A.p0, B.p0);
    const float a = nc::dot(A.d, A.d), e = nc::dot(B.d, B.d), b = nc::dot(A.d, B.d), c = nc::dot(A.d, r), f = nc::dot(B.d, r);
    const float ae = a * e, den = ae - b * b;
    nrm = mk(0, 0, 0); cnd = make_float4(0, 0, 0, 0);
    if (!(den > 1e-4f * ae)) return false;
    const float s = (b * f - c * e) / den, t = (a * f - b * c) / den;
    if (!(s > 0 && s < 1 && t > 0 && t < 1)) return false;
    const v3 p = nc::add(A.p0, nc::scale(A.d, s)), q = nc::add(B.p0, nc::scale(B.d, t));
    const v3 nv = nc::cross(A.d, B.d);
    const float il = 1.0f / sqrtf(nc::dot(nv, nv));
    const float sg = nc::dot(nv, nc::add(A.n1, A.n2)) > 0 ? il : -il;
    const v3 u = nc::scale(nv, sg);
    if (!(nc::dot(nc::cross(A.n1, u), nc::cross(u, A.n2)) >= 0)) return false;
    const v3 w = nc::scale(u, -1.0f);
    if (!(nc::dot(w, nc::add(B.n1, B.n2)) > 0)) return false;
    if (!(nc::dot(nc::cross(B.n1, w), nc::cross(w, B.n2)) >= 0)) return false;
    const v3 pq = nc::sub(p, q);
    const float dist = nc::dot(w, pq);
    if (!(dist < margin && dist > -0.005f && dist > lo)) return false;      // (oracle EDGE_DEPTH; lo: not deeper than the face axes)
    const v3 x = nc::add(q, nc::scale(pq, 0.5f));
    cnd = make_float4(x.x, x.y, x.z, dist);
    nrm = w;
    return true;
}
// index of the first maximum of val(i) over the candidates i < n with ok(i), or -1 when there is none above `floor_`;
// candidates are visited 64 at a time, a later chunk only replaces the winner when it is strictly greater
#define CAND_ARGMAX(RESULT, FLOOR, OKEXPR, VALEXPR)                                                   \
    {                                                                                                 \
        float bestv_ = (FLOOR); int besti_ = -1;                                                      \
        for (int c0_ = 0; c0_ < ncand; c0_ += 64) {                                                   \
            const int ci = c0_ + lane;                                                                \
            const bool in_ = ci < ncand;                                                              \
            const float4 ca = cand_a[in_ ? ci : 0];                                                   \
            const bool ok_ = in_ && (OKEXPR);                                                         \
            const float val_ = (VALEXPR);                                                             \
            const float m_ = wave_max(ok_ ? val_ : -3.0e38f);                                         \
            if (m_ > bestv_) {                                                                        \
                const unsigned long long bb_ = __ballot(ok_ && val_ == m_);                           \
                if (bb_) { bestv_ = m_; besti_ = c0_ + __ffsll((long long)bb_) - 1; }                 \
            }                                                                                         \
        }                                                                                             \
        RESULT = besti_;                                                                              \
    }
// The collision pass of one env: reads the contact history (current frame: D.clist, D.ccount, D.cforce) and the collision
// inputs prep_body<1> left in the scratch slab, fills the NEXT frame (D.clist_next, D.ccount_next, D.cwarm_next, class + lists).
__device__ __forceinline__ void collide_env(const SimParams &P, const DevPtrs &D, int ns, int env) {
    const int N = P.N;
    const float *state = D.state;
    float *scratch = D.scratch;
    if (D.errflags[env] & 1u) {         // frozen env: no contacts, light
        if (threadIdx.x == 0) { D.ccount_next[env] = 0; D.hgflag_next[env] = 0; }
        return;
    }
    const ShapeData *S = D.shapes;
    // 38.9 KB of LDS: four workgroups = sixteen waves per CU
    __shared__ float xf[CSHAPES][12];          // R (row-major 9), p (3) of every shape's owner
    __shared__ float4 sph[CSHAPES];            // world bounding sphere
    __shared__ float sroff[CSHAPES];           // radius of the shape grown by the margin plane by plane (ShapeData::roff)
    __shared__ float4 pre_pl[CSHAPES][NPREF];  // the leading planes of every shape (its extreme facets), owner frame: the pair cull of the broad phase
    __shared__ int pair_ab[MAXPAIRS];          // shape a | shape b << 8 of every pair   } staged once: no global load of
    __shared__ int shape_n[CSHAPES];           // vertex count | plane count << 8 | edge count << 16   } metadata inside the pair loop
    __shared__ int pair_key[MAXPAIRS];         // bodyA | bodyB << 8 | link of shape a << 16 (the meta word of the pair's contacts)
    __shared__ unsigned char edge_id[COLLIDE_WAVES][2][EMAXC];   // per wave: the original indices of the staged edges
    __shared__ unsigned char close_pair[MAXPAIRS];   // the pairs that pass the sphere test, in pair order
    __shared__ int n_close, next_item, nct_sh;
    __shared__ float4 res_a[CCHUNK][4];        // per close pair of the chunk: the kept candidates (contact point, signed distance)
    __shared__ int res_b[CCHUNK][4];           //                              plane of "other" | direction << 8
    __shared__ int res_k[CCHUNK];              //                              their number; after the scan: offset in the env's list | kept << 8
    __shared__ int res_key[CCHUNK];            //                              bodyA | bodyB << 8 | linkA << 16 of the pair
    // per wave:
    __shared__ float4 planes_w[COLLIDE_WAVES][FMAXC];      // planes of "other" in the current direction
    __shared__ float surv_w[COLLIDE_WAVES][VMAXC][3];      // world position of the vertices that survive the prefilter, in vertex order
    __shared__ float4 cand_a_w[COLLIDE_WAVES][CAND_MAX];   // candidates of the pair: contact point, signed distance
    __shared__ unsigned short cand_b_w[COLLIDE_WAVES][CAND_MAX];   //                 plane of "other" it is nearest to | direction << 8; edge candidates: edge of a | edge of b << 6 | 1 << 15
    __shared__ float4 pv[MAXC];                // contact history (warm start): {x, y, z, normal force} of the previous step's contacts,
    __shared__ int pv_key[MAXC];               //   their bodyA | bodyB << 8 | linkA << 16 | pair << 24,
    __shared__ unsigned char run_s[MAXPAIRS], run_e[MAXPAIRS];   //   and per pair its run [start, end) of that list
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float4 *planes = planes_w[wv];
    float (*surv)[3] = surv_w[wv];
    float4 *cand_a = cand_a_w[wv];
    unsigned short *cand_b = cand_b_w[wv];
    CPROF_INIT
    const int nprev = P.warmstart > 0.0f ? min(D.ccount[env], MAXC) : 0;      // contacts of the step before (the current frame; this pass fills the next one)
    for (int pr = tid; pr < P.npairs; pr += COLLIDE_THREADS) {
        const int ba = S->pair_meta[pr][0], bb = S->pair_meta[pr][1];
        const int cls = (((ba >= 0 && ba < 16) || (bb >= 0 && bb < 16)) ? 1 : 0) | ((ba >= 16 && bb >= 16) ? 2 : 0);
        pair_key[pr] = (ba & 255) | ((bb & 255) << 8) | ((S->pair_meta[pr][2] & 255) << 16);
        pair_ab[pr] = S->pair_a[pr] | (S->pair_b[pr] << 8) | (cls << 16) | (bb < 0 ? 1 << 18 : 0);      // + robot involved (bit 16), object-object (bit 17), b static (bit 18)
    }
    if (wv == 1) {       // the contact history comes in with the same round trip as the shape transforms (it has left the L2 since k_solve read it)
        for (int q = lane; q < MAXPAIRS; q += 64) { run_s[q] = 0; run_e[q] = 0; }
        if (lane < nprev) {
            const float4 *pr_ = D.clist + ((size_t)env * MAXC + lane) * 3;
            const float4 p0 = pr_[0], p1 = pr_[1];
            pv[lane] = make_float4(p0.x, p0.y, p0.z, D.cforce[(size_t)env * MAXC + lane]);
            pv_key[lane] = __float_as_int(p1.w);
        }
        CSYNC();
        if (lane < nprev) {       // the list is in pair order: the contacts of a pair form one run
            const int pj = pv_key[lane] >> 24;
            if (lane == 0 || (pv_key[lane - 1] >> 24) != pj) run_s[pj] = (unsigned char)lane;
            if (lane + 1 >= nprev || (pv_key[lane + 1] >> 24) != pj) run_e[pj] = (unsigned char)(lane + 1);
        }
    }
    if (tid < ns) {
        shape_n[tid] = S->nv[tid] | (S->nf[tid] << 8) | (S->ne[tid] << 16);
        const Xf X = load_xf(S, tid, scratch, env);
#pragma unroll
        for (int k = 0; k < 9; k++) xf[tid][k] = X.R.m[k];
        xf[tid][9] = X.p.x; xf[tid][10] = X.p.y; xf[tid][11] = X.p.z;
        const v3 c = nc::add(nc::mulv(X.R, mk(S->sphere[tid][0], S->sphere[tid][1], S->sphere[tid][2])), X.p);
        sph[tid] = make_float4(c.x, c.y, c.z, S->sphere[tid][3]);
        sroff[tid] = S->roff[tid];
    }
    if (tid < ns * NPREF) { const int s_ = tid / NPREF, f_ = tid - s_ * NPREF; pre_pl[s_][f_] = *(const float4 *)S->planes[s_][f_]; }
    __syncthreads();
    CPROF(0);
    if (CABL(256)) return;
    // ---- the pairs whose bounding spheres come within the margin, in pair order (wave 0)
    if (wv == 0) {
        int nc_ = 0;
        for (int p0 = 0; p0 < P.npairs; p0 += 64) {
            const int pr = p0 + lane;
            bool close = false;
            if (pr < P.npairs) {
                const float4 a = sph[pair_ab[pr] & 255], b = sph[(pair_ab[pr] >> 8) & 255];
                const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, rr = a.w + b.w + P.margin;
                close = !(dx * dx + dy * dy + dz * dz > rr * rr);
                // Pair cull: a shape GROWN BY THE MARGIN PLANE BY PLANE (the set a vertex must reach to become a candidate) lies inside
                // the ball of radius roff about its sphere centre; when that ball is beyond one plane of the other shape, no vertex of
                // either shape is a candidate and no edge pair comes within the margin -- the pair yields nothing in the oracle's
                // collide_pair(), whatever its three passes compute.  Here against the other shape's six leading planes (conservative
                // arithmetic: roff carries its own slack).  (Repeating it against ALL planes in direction 0's exact cull, with a way out of the
                // pair there, was built too: the extra exit costs 10 spilled registers and the leading planes catch nearly all of it.)
                if (close) {
#pragma unroll
                    for (int d_ = 0; d_ < 2; d_++) {
                        const int sm_ = d_ ? (pair_ab[pr] >> 8) & 255 : pair_ab[pr] & 255, so_ = d_ ? pair_ab[pr] & 255 : (pair_ab[pr] >> 8) & 255;
                        const float4 cm_ = d_ ? b : a;
                        const float *xo = xf[so_];
                        const float ex = cm_.x - xo[9], ey = cm_.y - xo[10], ez = cm_.z - xo[11];
                        const float lx = xo[0] * ex + xo[3] * ey + xo[6] * ez, ly = xo[1] * ex + xo[4] * ey + xo[7] * ez, lz = xo[2] * ex + xo[5] * ey + xo[8] * ez;
                        const float lim = sroff[sm_] + 1e-5f;
#pragma unroll
                        for (int f_ = 0; f_ < NPREF; f_++) {
                            const float4 pl = pre_pl[so_][f_];
                            if (pl.x * lx + pl.y * ly + pl.z * lz - pl.w > lim) close = false;
                        }
                    }
                }
            }
            const unsigned long long cm_ = CABL(512) ? 0ull : __ballot(close);
            if (close && !CABL(512)) close_pair[nc_ + lanes_below(cm_)] = (unsigned char)pr;
            nc_ += __popcll(cm_);
        }
        if (lane == 0) { n_close = nc_; next_item = 0; }
    }
    __syncthreads();
    CPROF(1);
    const int ncl = n_close;
    int nct = 0;                                // contacts of this env so far        }
    int ngen = 0;                               // contacts that are not object-vs-static ones the object lanes take: generic rows    } tracked by wave 0
    int oscnt0 = 0, oscnt1 = 0, oscnt2 = 0;     // object-vs-static contacts per object }
    int nchunk = 0;
    for (int base = 0; base < ncl && nct < MAXC; base += nchunk) {
        nchunk = min(CCHUNK, ncl - base);
        // (more than CCHUNK close pairs: rare) the pairs of one moving shape with the statics share their bodies -- the warm
        // start below looks at all contacts of the same bodies, so a chunk never ends inside such a run (<= 3 pairs)
        while (base + nchunk < ncl) {
            const int pa_ = pair_ab[close_pair[base + nchunk - 1]], pb_ = pair_ab[close_pair[base + nchunk]];
            if ((pa_ & 255) == (pb_ & 255) && (pa_ & pb_ & (1 << 18))) nchunk--; else break;
        }
        // ---- every wave takes the next unprocessed close pair of the chunk (the result goes to the pair's slot: the
        // outcome does not depend on which wave took it)
        for (;;) {
            int item = 0;
            if (lane == 0) item = atomicAdd(&next_item, 1);
            item = __builtin_amdgcn_readfirstlane(item);
            if (item >= base + nchunk) break;
            CPROF_COUNT(7);
            const int slot = item - base;
            const int pair = close_pair[item];
            const int sa = pair_ab[pair] & 255, sb = (pair_ab[pair] >> 8) & 255;
            int ncand = 0;                      // wave-uniform
            bool apart = false;                 // the exact cull of a direction found the shapes more than the margin apart
            // the global loads of a direction -- the planes of "other" (lane = plane, three per lane) and the vertices of "mine" (lane =
            // vertex, three passes) -- are issued one direction ahead: those of direction 0 here, those of direction 1 as soon as
            // direction 0 has staged its planes (their round trip hides behind its prefilter and all-plane pass)
            float4 plr2[2][FMAXC / 64];
            float vxr2[2][VMAXC / 64], vyr2[2][VMAXC / 64], vzr2[2][VMAXC / 64];
#define COLLIDE_LOADS(d)                                                                                                  \
            {                                                                                                             \
                const int sm_ = (d) ? sb : sa, so_ = (d) ? sa : sb;                                                       \
                _Pragma("unroll") for (int i = 0; i < FMAXC / 64; i++) plr2[d][i] = *(const float4 *)S->planes[so_][min(lane + 64 * i, FMAXC - 1)]; \
                _Pragma("unroll") for (int i = 0; i < VMAXC / 64; i++) {                                                  \
                    const float *vp = S->verts[sm_][min(lane + 64 * i, VMAXC - 1)];                                       \
                    vxr2[d][i] = vp[0]; vyr2[d][i] = vp[1]; vzr2[d][i] = vp[2];                                           \
                }                                                                                                         \
            }
            COLLIDE_LOADS(0)
#pragma unroll
            for (int dirflag = 0; dirflag < 2; dirflag++) {
                // "mine" = the shape whose vertices are tested, "other" = the shape whose planes they are tested against
                const int sm = dirflag ? sb : sa, so = dirflag ? sa : sb;
                Xf Xm, Xo;
#pragma unroll
                for (int kk = 0; kk < 9; kk++) { Xm.R.m[kk] = xf[sm][kk]; Xo.R.m[kk] = xf[so][kk]; }
                Xm.p = mk(xf[sm][9], xf[sm][10], xf[sm][11]);
                Xo.p = mk(xf[so][9], xf[so][10], xf[so][11]);
                const int nv = shape_n[sm] & 255, nf = (shape_n[so] >> 8) & 255;
                float4 (&plr)[FMAXC / 64] = plr2[dirflag];
                float (&vxr)[VMAXC / 64] = vxr2[dirflag], (&vyr)[VMAXC / 64] = vyr2[dirflag], (&vzr)[VMAXC / 64] = vzr2[dirflag];
                CSYNC();            // the previous direction's reads of planes / surv are done
                bool sep = false;
                {   // a. exact cull + b. plane staging (lane = plane)
                    const float4 cm = sph[sm];
                    const v3 cl = nc::tmulv(Xo.R, nc::sub(mk(cm.x, cm.y, cm.z), Xo.p));
#pragma unroll
                    for (int i = 0; i < FMAXC / 64; i++) {
                        const int f = lane + 64 * i;
                        if (f < nf) {
                            const float4 pl = plr[i];
                            planes[f] = pl;
                            sep = sep || (pl.x * cl.x + pl.y * cl.y + pl.z * cl.z - pl.w > cm.w + P.margin);
                        }
                    }
                }
                if (dirflag == 0) COLLIDE_LOADS(1)
                CPROF(2);
                if (__ballot(sep)) { if (!apart) CPROF_COUNT(8 + dirflag); apart = true; continue; }
                if (CABL(1024)) continue;
                CSYNC();
                const int npre = min(NPREF, nf);
                int nsurv = 0;                  // wave-uniform
#pragma unroll
                for (int i = 0; i < VMAXC / 64; i++) {
                    if (64 * i >= nv) break;
                    const int v = 64 * i + lane;
                    bool keep = false;
                    v3 xw = mk(0, 0, 0);
                    if (v < nv) {
                        xw = nc::mulv_add_fma(Xm.R, mk(vxr[i], vyr[i], vzr[i]), Xm.p);
                        const v3 xl = nc::tmulv_fma(Xo.R, nc::sub(xw, Xo.p));
                        float best = -1e30f;
                        for (int f = 0; f < npre; f++) best = fmaxf(best, nc::plane_dist_fma(planes[f], xl));
                        keep = best < P.margin;
                    }
                    const unsigned long long km = __ballot(keep);
                    if (keep) {
                        const int pos = nsurv + lanes_below(km);
                        surv[pos][0] = xw.x; surv[pos][1] = xw.y; surv[pos][2] = xw.z;
                    }
                    nsurv += __popcll(km);
                }
                CPROF(3);
                if (nsurv == 0) continue;
                CSYNC();
                // Lane = survivor, every plane -- or, where that is shorter, EIGHT lanes per survivor, each with every eighth plane, and
                // three exchange steps that keep the larger distance (of equal ones the lower plane index: a sequential loop's "first
                // maximum wins").  A handful of an arm link's vertices near a 192-plane hull: nf / 8 iterations instead of nf; forty
                // vertices of an object inside the table's six planes: one round of six as before.  (Costs in instructions: seven per
                // plane, 55 / 80 per round.)
                {
                    const int wide_cost = ((nsurv + 7) >> 3) * (((nf + 7) >> 3) * 7 + 80), lane_cost = ((nsurv + 63) >> 6) * (nf * 7 + 55);
                    const int lg = wide_cost < lane_cost ? 3 : 0;          // wave-uniform
                    const int sub = lane & ((1 << lg) - 1);
                    for (int k0 = 0; k0 < nsurv; k0 += 64 >> lg) {
                        const int k = k0 + (lane >> lg);
                        const bool valid = k < nsurv;
                        const int kk = valid ? k : 0;
                        const v3 xw = mk(surv[kk][0], surv[kk][1], surv[kk][2]);
                        const v3 xl = nc::tmulv_fma(Xo.R, nc::sub(xw, Xo.p));
                        float best = -1e30f;
                        int bf = 0;
                        for (int f = sub; f < nf; f += 1 << lg) {
                            const float sd = nc::plane_dist_fma(planes[f], xl);
                            if (sd > best) { best = sd; bf = f; }
                        }
                        if (lg) {
#define XCH_MAX(CTRL) { const float ob_ = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best), (CTRL), 0xf, 0xf, false));   \
                        const int of_ = __builtin_amdgcn_update_dpp(0, bf, (CTRL), 0xf, 0xf, false);                                        \
                        const bool take_ = ob_ > best || (ob_ == best && of_ < bf); best = take_ ? ob_ : best; bf = take_ ? of_ : bf; }
                            XCH_MAX(0xB1) XCH_MAX(0x4E) XCH_MAX(0x141)      // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror (the other quad of the eight)
#undef XCH_MAX
                        }
                        const bool hit = valid && sub == 0 && best < P.margin;
                        const unsigned long long hm = __ballot(hit);
                        const int pos = ncand + lanes_below(hm);
                        if (hit && pos < CAND_MAX) {
                            const float4 pl = planes[bf];
                            const v3 nw = nc::mulv(Xo.R, mk(pl.x, pl.y, pl.z));
                            cand_a[pos] = make_float4(xw.x - 0.5f * best * nw.x, xw.y - 0.5f * best * nw.y, xw.z - 0.5f * best * nw.z, best);
                            cand_b[pos] = (unsigned short)(bf | (dirflag << 8));
                        }
                        ncand = min(ncand + __popcll(hm), CAND_MAX);
                    }
                }
                CPROF(4);
            }
            CSYNC();
            // ---- edge-edge candidates (oracle edge_edge()): two edges crossing away from any vertex.  Lane = edge: the long sharp edges of both shapes go to the world frame, those that come
            // within the margin of the other shape's bounding sphere are staged in LDS (planes: A's, surv: B's; in index
            // order); then lane = edge pair, in the oracle's (i, j) order.
            const int ne_a = shape_n[sa] >> 16, ne_b = shape_n[sb] >> 16;
            if (!apart && ne_a > 0 && ne_b > 0 && P.edge_contacts && !CABL(1024)) {
                int nst[2];
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    const int sm = side ? sb : sa, so = side ? sa : sb, ne = side ? ne_b : ne_a;
                    bool keep = false;
                    EdgeW E;
                    if (lane < ne) {
                        E = edge_world(S->edges[sm][lane], xf[sm]);
                        // conservative: a contact needs a point of this edge within radius + margin of the other sphere's centre
                        const float4 co = sph[so];
                        const v3 r0 = nc::sub(mk(co.x, co.y, co.z), E.p0);
                        const float dd = nc::dot(E.d, E.d);
                        float tt = nc::dot(r0, E.d) / dd;
                        tt = fminf(fmaxf(tt, 0.0f), 1.0f);
                        const v3 rr = nc::sub(r0, nc::scale(E.d, tt));
                        const float lim = co.w + P.margin;
                        keep = nc::dot(rr, rr) <= lim * lim * 1.01f + 1e-6f;
                    }
                    const unsigned long long km = __ballot(keep);
                    if (keep) {
                        const int pos = lanes_below(km);
                        float4 *dst = side ? (float4 *)&surv[0][0] + 3 * pos : planes + 3 * pos;
                        dst[0] = make_float4(E.p0.x, E.p0.y, E.p0.z, E.d.x);
                        dst[1] = make_float4(E.d.y, E.d.z, E.n1.x, E.n1.y);
                        dst[2] = make_float4(E.n1.z, E.n2.x, E.n2.y, E.n2.z);
                        edge_id[wv][side][pos] = (unsigned char)lane;
                    }
                    nst[side] = __popcll(km);
                }
                CSYNC();
                // overlapping shapes: an edge axis deeper than the deepest vertex candidate (the face axes) is no contact
                float smin = 0.0f;
                for (int c0_ = 0; c0_ < ncand; c0_ += 64) smin = fminf(smin, -wave_max(c0_ + lane < ncand ? -cand_a[c0_ + lane].w : -3.0e38f));
                const float lo = smin - 0.0005f;                 // (oracle EDGE_SLOP)
                const int na = nst[0], nb = nst[1], npairs_e = na * nb;
                const float inb = 1.0f / (float)nb;
                for (int k0 = 0; k0 < npairs_e; k0 += 64) {
                    const int kk = k0 + lane;
                    bool hit = false;
                    float4 cnd = make_float4(0, 0, 0, 0);
                    int ids = 0;
                    if (kk < npairs_e) {
                        const int i = (int)(((float)kk + 0.5f) * inb), j = kk - i * nb;      // exact for these small integers
                        const float4 *pa = planes + 3 * i, *pb = (const float4 *)&surv[0][0] + 3 * j;
                        const float4 a0 = pa[0], a1_ = pa[1], a2_ = pa[2], b0 = pb[0], b1_ = pb[1], b2_ = pb[2];
                        EdgeW A, B;
                        A.p0 = mk(a0.x, a0.y, a0.z); A.d = mk(a0.w, a1_.x, a1_.y); A.n1 = mk(a1_.z, a1_.w, a2_.x); A.n2 = mk(a2_.y, a2_.z, a2_.w);
                        B.p0 = mk(b0.x, b0.y, b0.z); B.d = mk(b0.w, b1_.x, b1_.y); B.n1 = mk(b1_.z, b1_.w, b2_.x); B.n2 = mk(b2_.y, b2_.z, b2_.w);
                        v3 nrm;
                        hit = edge_pair(A, B, P.margin, lo, cnd, nrm);
                        ids = edge_id[wv][0][i] | (edge_id[wv][1][j] << 6) | (1 << 15);
                    }
                    const unsigned long long hm = __ballot(hit);
                    const int pos = ncand + lanes_below(hm);
                    if (hit && pos < CAND_MAX) { cand_a[pos] = cnd; cand_b[pos] = (unsigned short)ids; }
                    ncand = min(ncand + __popcll(hm), CAND_MAX);
                }
                CSYNC();
            }
            // manifold reduction, same rule as the oracle's reduce4(): deepest first, then maximal spread, preferring the
            // candidates within TIER_TOL (1 mm) of the deepest penetration at every pick; ties go to the first candidate
            int sel0 = -1, sel1 = -1, sel2 = -1, sel3 = -1, k = 0;
            if (CABL(2048)) ncand = 0;
            if (ncand <= 4) {
                sel0 = ncand > 0 ? 0 : -1; sel1 = ncand > 1 ? 1 : -1; sel2 = ncand > 2 ? 2 : -1; sel3 = ncand > 3 ? 3 : -1;
                k = ncand;
            } else {
                CAND_ARGMAX(sel0, -3.0e38f, true, -ca.w)                       // smallest s, first one
                const float smin = cand_a[sel0].w, lim = smin + 0.001f, tie = smin + 0.0005f;
                // anchor = a candidate within TIE_TOL (0.5 mm) of the deepest (oracle reduce4(): a resting face must give
                // the same quadruple whichever of its vertices happens to be deepest by a micrometre)
                // -- and among those the extreme one along a fixed skew direction, i.e. a corner of the face
                CAND_ARGMAX(sel0, -3.0e38f, ca.w < tie, ca.x + 0.618f * ca.y + 0.382f * ca.z)
                const float4 c0 = cand_a[sel0];
                const v3 x0 = mk(c0.x, c0.y, c0.z);
#define V1_ nc::dot(nc::sub(mk(ca.x, ca.y, ca.z), x0), nc::sub(mk(ca.x, ca.y, ca.z), x0))
                CAND_ARGMAX(sel1, -1.0f, ci != sel0 && ca.w < lim, V1_)
                if (sel1 < 0) CAND_ARGMAX(sel1, -1.0f, ci != sel0, V1_)
                const float4 c1 = cand_a[sel1];
                const v3 e = nc::sub(mk(c1.x, c1.y, c1.z), x0);
#define CR_ nc::cross(nc::sub(mk(ca.x, ca.y, ca.z), x0), e)
#define V2_ nc::dot(CR_, CR_)
                CAND_ARGMAX(sel2, -1.0f, ci != sel0 && ci != sel1 && ca.w < lim, V2_)
                if (sel2 < 0) CAND_ARGMAX(sel2, -1.0f, ci != sel0 && ci != sel1, V2_)
                const float4 c2 = cand_a[sel2];
                const v3 cr2 = nc::cross(nc::sub(mk(c2.x, c2.y, c2.z), x0), e);
#define V3_ (-nc::dot(CR_, cr2))
                CAND_ARGMAX(sel3, 0.0f, ci != sel0 && ci != sel1 && ci != sel2 && ca.w < lim, V3_)
                if (sel3 < 0) CAND_ARGMAX(sel3, 0.0f, ci != sel0 && ci != sel1 && ci != sel2, V3_)
#undef V1_
#undef CR_
#undef V2_
#undef V3_
                k = sel3 >= 0 ? 4 : 3;
            }
            if (lane < k) {
                const int ci = lane == 0 ? sel0 : (lane == 1 ? sel1 : (lane == 2 ? sel2 : sel3));
                res_a[slot][lane] = cand_a[ci];
                res_b[slot][lane] = cand_b[ci];
            }
            if (lane == 0) res_k[slot] = k;
            if (!apart && ncand == 0) CPROF_COUNT(10);
            if (k > 0) CPROF_COUNT(11);
            CSYNC();            // the candidate list is reused by the next pair
            CPROF(5);
        }
        __syncthreads();
        // ---- the chunk's contacts go to the env's list in pair order, up to MAXC (the oracle stops there too): wave 0
        // numbers them and classifies the env's solver group, then thread (slot, r) writes the slot's r-th record
        if (wv == 0) {
            const bool in_ = lane < nchunk;
            const int kj = in_ ? res_k[lane] : 0;
            int total;
            const int off = min(nct + wave_excl_scan(kj, lane, total), MAXC);
            const int kk = min(kj, MAXC - off);
            if (in_) {
                res_k[lane] = off | (kk << 8);
                res_key[lane] = pair_key[close_pair[base + lane]];
            }
            // the solver's object lanes take up to four object-vs-static contacts per object; anything else is a generic row
            const int pab = pair_ab[close_pair[base + (in_ ? lane : 0)]];
            const int cls = (pab >> 16) & 3;
            const int ob = (pab & 255) - (ns - NOBJ);                   // object index of shape a for the object-vs-static pairs
            const bool os = cls == 0 && ob >= 0;
            { int tg_; wave_excl_scan(os ? 0 : kk, lane, tg_); ngen += tg_; }
            int t0_, t1_, t2_;
            wave_excl_scan(os && ob == 0 ? kk : 0, lane, t0_);
            wave_excl_scan(os && ob == 1 ? kk : 0, lane, t1_);
            wave_excl_scan(os && ob == 2 ? kk : 0, lane, t2_);
            oscnt0 += t0_; oscnt1 += t1_; oscnt2 += t2_;
            nct = min(nct + total, MAXC);
        }
        __syncthreads();
        {
            const int slot = tid >> 2, r = tid & 3;
            const int ok_ = slot < nchunk ? res_k[slot] : 0;
            if (r < (ok_ >> 8)) {
                const int pair = close_pair[base + slot];
                const int sa = pair_ab[pair] & 255, sb = (pair_ab[pair] >> 8) & 255;
                const float4 a = res_a[slot][r];
                // the normal (B -> A) of a kept candidate: its plane of "other", rotated to the world, as in the candidate test
                const int kb = res_b[slot][r];
                v3 nb;
                if (kb >> 15) {       // edge-edge candidate: the common normal of edge (kb & 63) of a and edge (kb >> 6 & 63) of b, as in the test
                    float4 dummy;
                    edge_pair(edge_world(S->edges[sa][kb & 63], xf[sa]), edge_world(S->edges[sb][(kb >> 6) & 63], xf[sb]), P.margin, -1.0f, dummy, nb);
                } else {
                    const int so_ = (kb >> 8) ? sa : sb;
                    m3 Ro;
#pragma unroll
                    for (int kk = 0; kk < 9; kk++) Ro.m[kk] = xf[so_][kk];
                    const float4 pl = *(const float4 *)S->planes[so_][kb & 255];
                    nb = nc::mulv(Ro, mk(pl.x, pl.y, pl.z));
                    if (kb >> 8) nb = nc::scale(nb, -1.0f);
                }
                const float4 b = make_float4(nb.x, nb.y, nb.z, 0.0f);
                const int meta = pair_key[pair];
                float4 *rec = D.clist_next + ((size_t)env * MAXC + (ok_ & 255) + r) * 3;
                rec[0] = make_float4(a.x, a.y, a.z, b.x);
                rec[1] = make_float4(b.y, b.z, a.w, __int_as_float(meta | (pair << 24)));      // (bits 24..30: the pair, for the next step's matching)
                rec[2] = D.pair_mat[(size_t)env * P.npairs + pair];       // (the env's own materials: rr_set_object_dynamics)
                // warm start (oracle warm_start_match()): the previous contact of the same bodies nearest to this one within the
                // margin, unless another new contact of those bodies is nearer to it (or as near and earlier in the list).
                // Pairs with the same bodies -- a moving shape against the statics -- are at most three consecutive ones, so
                // their contacts form one range of the previous list and one range of slots; all LDS reads of a stage are
                // issued together (a chain of dependent LDS round trips at the kernel's tail costs more than the arithmetic).
                float lam0 = 0.0f;
                {
                    const v3 x = mk(a.x, a.y, a.z);
                    const int key = meta, me = (ok_ & 255) + r;
                    int J0 = MAXC, J1 = 0;
                    {
                        int kq[5], rs[5], re[5];
#pragma unroll
                        for (int u = 0; u < 5; u++) {
                            const int q = min(max(pair - 2 + u, 0), P.npairs - 1);
                            kq[u] = pair_key[q]; rs[u] = run_s[q]; re[u] = run_e[q];
                        }
#pragma unroll
                        for (int u = 0; u < 5; u++) if (kq[u] == key && re[u] > rs[u]) { J0 = min(J0, rs[u]); J1 = max(J1, re[u]); }
                    }
                    int bj = -1;
                    float bd = 0.0004f;
                    for (int j0_ = J0; j0_ < J1; j0_ += 4) {
                        float4 pj[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) pj[u] = pv[min(j0_ + u, MAXC - 1)];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const v3 d = nc::sub(x, mk(pj[u].x, pj[u].y, pj[u].z));
                            const float d2 = nc::dot(d, d);
                            if (j0_ + u < J1 && d2 < bd) { bd = d2; bj = j0_ + u; }
                        }
                    }
                    if (bj >= 0) {
                        const float4 pb = pv[bj];
                        int k2[5], o2[5];
#pragma unroll
                        for (int u = 0; u < 5; u++) {
                            const int s2 = min(max(slot - 2 + u, 0), nchunk - 1);
                            k2[u] = res_key[s2]; o2[u] = res_k[s2];
                        }
                        bool heir = true;
#pragma unroll
                        for (int u = 0; u < 5; u++) {
                            const int s2 = slot - 2 + u;
                            if (s2 < 0 || s2 >= nchunk || k2[u] != key) continue;       // (wave-divergent, but the body's reads are issued together)
                            float4 a2[4];
#pragma unroll
                            for (int r2 = 0; r2 < 4; r2++) a2[r2] = res_a[s2][r2];
#pragma unroll
                            for (int r2 = 0; r2 < 4; r2++) {
                                const int other = (o2[u] & 255) + r2;
                                const v3 d = nc::sub(mk(a2[r2].x, a2[r2].y, a2[r2].z), mk(pb.x, pb.y, pb.z));
                                const float d2 = nc::dot(d, d);
                                if (r2 < (o2[u] >> 8) && other != me && (d2 < bd || (d2 == bd && other < me))) heir = false;
                            }
                        }
                        if (heir) lam0 = P.warmstart * (pb.w * P.dt);
                    }
                }
                D.cwarm_next[(size_t)env * MAXC + (ok_ & 255) + r] = lam0;
            }
        }
        CPROF(6);
        if (base + nchunk < ncl) {  // (more than CCHUNK close pairs: rare) the result slots are reused; every wave needs the count
            if (tid == 0) { nct_sh = nct; next_item = base + nchunk; }
            __syncthreads();
            nct = nct_sh;
        }
    }
    CPROF_END;
    if (tid == 0) {
        // "heavy": any generic contact (an env with a few generic rows lengthens its wave's chain by a quarter, an arm pressed on
        // the table fourfold; thresholds of 3 / 6 / 10 generic contacts were measured slower at every horizon but the longest)
        // generic contacts = all but the object-vs-static ones the solver's object lanes take: up to KOS = 4 per object and
        // P.os_cap in all, in list order (those pairs come first) -- the row builder's rule, so that a "light" env has none
        ngen = nct - min(P.os_cap, min(oscnt0, 4) + min(oscnt1, 4) + min(oscnt2, 4));
        const bool heavy = ngen > 0;
        D.ccount_next[env] = nct;
        // (the very heavy list is capped at VH_MAX entries -- its solve is launched with one wave per entry; beyond that an env is
        // just "heavy": classes are scheduling, never a result)
        bool vh = heavy && ngen > P.heavy2_min;
        if (vh) {
            const int sl = atomicAdd(D.hcount2_next, 1);
            if (sl < VH_MAX) { D.hgflag_next[env] = 2; D.hlist2_next[sl] = env; }
            else { atomicSub(D.hcount2_next, 1); vh = false; }
        }
        if (heavy && !vh) { const int sl = atomicAdd(D.hcount_next, 1); D.hgflag_next[env] = 1; D.hlist_next[sl] = env; }
        else if (!heavy) D.hgflag_next[env] = 0;
    }
}
// One workgroup per env.  `ordered` (all envs, sel 0): the workgroups take the envs in the order of D.collide_perm -- by falling
// duration of their last collision pass (dispatch_order_class, sorted by the extra workgroups of the preparation launch in front of
// this one; class x = the envs = x mod 8 = XCD x).  Measured (scratch/cwgtime.py, 4096 envs, four rounds of workgroups): the
// workgroups last 14 us (p90 17, p99 31, maximum 70); in env order -- even with last step's heavy envs first -- the shader engines
// take turns that free slots do not follow (0.67 of the slots busy, 700-800 of 1024 workgroups resident from the second round on)
// and the launch ends with whatever long env started last (90 us for 60 us of work).  Every env exactly once; the order is
// scheduling, never a result.  Otherwise (per-class launches, RR_COLLIDE_ORDER=0, batches of one round): pick_env.
#ifdef RR_RASTER_STATS
__device__ unsigned long long g_cwg_time[65536][3];
extern "C" int rr_debug_collide_wgtime(unsigned long long *out /*[65536][3]*/) { return (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cwg_time), sizeof(g_cwg_time)) == hipSuccess) ? 0 : -1; }
#endif
__global__ void __launch_bounds__(COLLIDE_THREADS, 4) k_collide(SimParams P, DevPtrs D, int ns, int sel, int ordered) {
    __shared__ unsigned s_tc0;            // (the start time waits in LDS, as in k_raster)
    if (threadIdx.x == 0) s_tc0 = (unsigned)__builtin_amdgcn_s_memrealtime();
    int env;
    if (ordered) { const unsigned it = D.collide_perm[blockIdx.x]; env = it == 0xffffffffu ? -1 : (int)(it >> 8); }
    else env = pick_env(D, sel, blockIdx.x, P.N);
    if (env < 0) return;
#ifdef RR_RASTER_STATS
    unsigned long long wt0_ = 0;      // (workgroup timeline of the collision pass: RR_ABLATE=131072, scratch/cwgtime.py)
    if (P.ablate & 0x20000) wt0_ = __builtin_amdgcn_s_memrealtime();
#endif
    collide_env(P, D, ns, env);
    if (threadIdx.x == 0) D.collide_cost[env] = (unsigned)__builtin_amdgcn_s_memrealtime() - s_tc0 + 1u;
#ifdef RR_RASTER_STATS
    if ((P.ablate & 0x20000) && threadIdx.x == 0) {
        unsigned long long *g = g_cwg_time[env & 65535];
        g[0] = wt0_; g[1] = __builtin_amdgcn_s_memrealtime();
        g[2] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11)) << 32);
    }
#endif
}
#undef CAND_ARGMAX
#undef COLLIDE_LOADS
#pragma clang fp contract(fast)
