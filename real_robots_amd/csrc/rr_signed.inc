// rr_signed.inc -- part of realrobot.hip (included there, behind rr_posture.inc; not a stand-alone translation unit).
// k_signed_distance: the SIGNED distance of every pair of the table (rr_set_distance_pairs) for the whole batch, at the present state
// or at K candidate joint postures per env (rr_signed_distance, realrobot.h).  Apart, a pair is what k_closest_points reports;
// overlapping, it gets minus the penetration depth -- the length of the shortest translation that separates the two convex hulls --,
// the direction of that translation, two witness points and a proved bound.  Read-only on the simulation (D.state, the model
// constants, the pair table and the tensor; never the preparation record); launched by rr_signed_distance alone, never by a step.
//
// One 256-thread workgroup per row (env, posture), grid N * K' exactly (K' = 1 at the present state); its four waves take every
// fourth pair, ONE WAVE64 PER PAIR.  Phases 1, 2 and 4 are k_posture_clearance's (the staged floats, the frames, the reduction to the
// row's first minimum through LDS behind the one barrier every wave reaches); the joints come from the tensor or, without one, from
// D.state.  A pair is steps a to c of rr_dist.inc's header RESTATED as sd_pair (running rr_dist.inc's text here was built and measured:
// this kernel went from 117 to 131 VGPRs, three waves per SIMD, and held to 128 by a launch bound it was 0.1 to 0.3 % slower on the
// collision table; so it keeps its copy: DESIGN.md), with two additions: the GJK tells its two status-1 exits apart -- the
// tetrahedron that holds the origin, or |v| <= DIST_TOUCH --, and at the first it hands over the tetrahedron: the three slots and w,
// each with its r = a_i - b_j about the sphere centres and its two vertex indices.
//
// d  THE EXPANSION (an expanding-polytope search on the Minkowski difference A - B, which holds the origin), on the same wave, all of
//    it wave-uniform and in a fixed order:
//    -- polytope vertex s lives in LANE s: r (about the centres; the point is r + cc) and the vertex indices (i of A, j of B); at most
//       4 + SD_TRIP_CAP = 36 of them.  A vertex comes out of its lane by v_readlane with a slot number made uniform and masked;
//    -- one polytope FACE PER LANE: three vertex slots in outward counter-clockwise order, the outward unit normal n and the plane
//       distance d = n . (r + cc) (a float64 sum of exact products, rounded once); the face cap is 64.  The normal comes from the
//       edges, differences of the r in which cc cancels.  A face whose normal cannot be formed (area^2 below 1e-10 of its edges'
//       product, the GJK's threshold) gets n = 0 and d = +inf: it is never the nearest and never visible, it only keeps the surface
//       closed;
//    -- a trip: the nearest live face F by a butterfly min over (d, lane), the lower lane among equals; the support w of A - B along
//       its normal (dist_support on A along n and on B along -n); n . w is the width of the hulls along n, an upper bound of the
//       depth that moving a by it along -n achieves, d_F a lower bound.  It ends, status 1, when n . w - d_F <= SD_EPS or when the
//       support pair (i, j) is already a polytope vertex (the GJK's "dup" rule: what ends the search exactly on coplanar vertex
//       sets).  Otherwise every lane tests its own face against w; __ballot gives the visible set (F is in it by construction); an
//       ordered loop over the ballot's bits crosses out, in every visible lane, the directed edges whose reverse belongs to a visible
//       face: what stays is the horizon.  The visible faces die, w takes the next vertex lane, and an ordered loop over the horizon
//       edges (edge number, then lane) gives each one the lowest free lane for the face (p, q, w).  More than 64 faces, or
//       SD_TRIP_CAP trips, ends with status 5: the best n . w seen and the nearest face's distance are still valid bounds;
//    -- the witness points are the barycentric weights (float64) of the origin's projection on a face of the final nearest plane -- of
//       the coplanar faces within SD_EPS of d_F, the lowest lane whose triangle holds the projection --, on the two shapes' support
//       vertices; the reported normal points from b towards a, against the face's outward one.
// No atomics, no LDS but the reduction's, fixed order: a row is a function of (env e's objects, its joints, the table) alone.  Loop
// bounds are constants, Q, or counts of ballot bits (at most 64); no value of the tensor or the state forms an address, vertex and
// slot indices come out of compares over lane numbers and are masked to the wave.
// With carried objects the kernel is k_posture_clearance's template <bool CARRY> over again (rr_posture.inc's header): <true> stages
// the objects behind one more barrier in phase 2 with carry_stage_object (rr_carry.inc), <false> is the text above and nothing else.
#define SD_THREADS 256
#define SD_WAVES (SD_THREADS / 64)
#define SD_PARK 20           // floats a wave parks: the record 0..11, key 12, j 13, status 14, body A 15, body B 16
#define SD_TRIP_CAP 32       // expansion trips per pair at most (status 5 behind them): 4 + 32 polytope vertices fit the wave's lanes
#define SD_EPS DIST_TOUCH    // m: the gap (n . w - d) between the depth's two bounds that ends the expansion

__device__ __forceinline__ float sd_lane(const float x, const int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
__device__ __forceinline__ v3 sd_lane(const v3 x, const int l) { return mk(sd_lane(x.x, l), sd_lane(x.y, l), sd_lane(x.z, l)); }
__device__ __forceinline__ int sd_slot(const int x, const int l) { return __builtin_amdgcn_readlane(x, l) & 63; }
// n . (r + cc): exact products, float64 sums, rounded once
__device__ __forceinline__ float sd_plane(const v3 n, const v3 r, const v3 cc) { return (float)(dist_ddot(n, r) + dist_ddot(n, cc)); }

// the face (A, B, C) in this winding: outward unit normal and plane distance; a face without a normal: n = 0, d = +inf
__device__ __forceinline__ void sd_face(const v3 A, const v3 B, const v3 C, const v3 cc, v3 *n, float *d) {
    // (float64: the edges are exact differences of the float32 r, so a sliver keeps the normal of the points it is made of; in float32
    // a rounding of 1e-7 of an edge over a corner angle of 1e-4 would turn the normal by 1e-3 rad)
    const double e1x = (double)B.x - A.x, e1y = (double)B.y - A.y, e1z = (double)B.z - A.z, e2x = (double)C.x - A.x, e2y = (double)C.y - A.y, e2z = (double)C.z - A.z;
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const double nn = cx * cx + cy * cy + cz * cz;
    const bool ok = nn > 1e-10 * (e1x * e1x + e1y * e1y + e1z * e1z) * (e2x * e2x + e2y * e2y + e2z * e2z);
    const double inv = 1.0 / sqrt(nn);
    const v3 u = mk((float)(cx * inv), (float)(cy * inv), (float)(cz * inv));
    *n = ok ? u : mk(0.0f, 0.0f, 0.0f);
    *d = ok ? sd_plane(u, A, cc) : INFINITY;
}

// the nearest live face: the lowest lane among equal distances, uniform in the wave
__device__ __forceinline__ int sd_nearest(const bool live, const float fd, const int lane) {
    float kv = live ? fd : INFINITY;
    int kl = lane;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float ov = __shfl_xor(kv, m);
        const int ol = __shfl_xor(kl, m);
        const bool take = ov < kv || (ov == kv && ol < kl);
        kv = take ? ov : kv;
        kl = take ? ol : kl;
    }
    return __builtin_amdgcn_readfirstlane(kl) & 63;
}

// One pair of the table for the 64 lanes of one wave; it returns the record's three float4, the status 0..5, the GJK's and the
// expansion's trips and the owners of the two shapes, the same values in every lane.
struct SdItem { float4 o0, o1, o2; int status, iters, trips, ota, oia, otb, oib; };
__device__ __forceinline__ SdItem sd_pair(const ShapeData *__restrict__ S, const DistTable *__restrict__ tab, const int j, const float *fr, const float *ob,
                                              const bool cull, const float maxd, const int lane) {
    // a.  (The table is validated by rr_set_distance_pairs; the clamps only keep the model's tables in range.)
    const int sa = min(max(__builtin_amdgcn_readfirstlane(tab->a[j]), 0), MAXSHAPES - 1), sb = min(max(__builtin_amdgcn_readfirstlane(tab->b[j]), 0), MAXSHAPES - 1);
    const int ota = S->otype[sa], otb = S->otype[sb];
    const int oia = min(max(S->oidx[sa], 0), ota == 2 ? NOBJ - 1 : NB - 1), oib = min(max(S->oidx[sb], 0), otb == 2 ? NOBJ - 1 : NB - 1);
    m3 Ra, Rb; v3 pa, pb;
    ray_shape_frame(ota, oia, fr, ob, &Ra, &pa);
    ray_shape_frame(otb, oib, fr, ob, &Rb, &pb);
    const v3 sca = mk(S->sphere[sa][0], S->sphere[sa][1], S->sphere[sa][2]), scb = mk(S->sphere[sb][0], S->sphere[sb][1], S->sphere[sb][2]);
    const v3 ca = mulv(Ra, sca) + pa, cb = mulv(Rb, scb) + pb;
    const float ra = S->sphere[sa][3], rb = S->sphere[sb][3];
    const v3 cc = ca - cb;
    const float cn = sqrtf(dot(cc, cc));
    const float gap = cn - ra - rb;
    float4 o0, o1, o2;
    int status, iters = 0, trips = 0;
    if (cull && gap > maxd) {
        const v3 u = cc * (1.0f / cn);
        const v3 xa = ca - u * ra, xb = cb + u * rb;
        status = 2;
        o0 = make_float4(gap, gap, xa.x, xa.y); o1 = make_float4(xa.z, xb.x, xb.y, xb.z); o2 = make_float4(u.x, u.y, u.z, 0.0f);
    } else {
        // b
        v3 xa[DIST_TRIPS], xb[DIST_TRIPS];
        const int nva = min(max(S->nv[sa], 1), VMAXC), nvb = min(max(S->nv[sb], 1), VMAXC);
#pragma unroll
        for (int t = 0; t < DIST_TRIPS; t++) {
            const int ka = min(64 * t + lane, nva - 1), kb = min(64 * t + lane, nvb - 1);
            xa[t] = mulv(Ra, mk(S->verts[sa][ka][0], S->verts[sa][ka][1], S->verts[sa][ka][2]) - sca);
            xb[t] = mulv(Rb, mk(S->verts[sb][kb][0], S->verts[sb][kb][1], S->verts[sb][kb][2]) - scb);
        }
        // c.  The simplex: three slots {r = a - b about the centres (the point is r + cc), a, b, the two vertex indices, weight}; weight 0: the slot is free.
        v3 sr[3], sA[3], sB[3];
        int ia[3], ib[3];
        float lam[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 3; k++) { sr[k] = sA[k] = sB[k] = mk(0.0f, 0.0f, 0.0f); ia[k] = ib[k] = -1; }
        v3 v = cn > 0.0f ? cc : mk(1.0f, 0.0f, 0.0f);             // the first direction: between the sphere centres (no point of the simplex yet)
        double vv = INFINITY;
        float lower = 0.0f;
        bool tet = false;                                         // the search ended on a tetrahedron that holds the origin: slots 0..2 and (tr, tja, tjb)
        v3 tr = mk(0.0f, 0.0f, 0.0f);
        int tja = 0, tjb = 0;
        status = 3;
        for (int it = 0; it < DIST_ITER_CAP; it++) {
            iters = it + 1;
            const int ja = dist_support(xa, v * -1.0f, lane), jb = dist_support(xb, v, lane);
            const v3 wa = dist_fetch(xa[0], xa[1], xa[2], ja), wb = dist_fetch(xb[0], xb[1], xb[2], jb);
            const v3 r = wa - wb, w = r + cc;
            const double vw = dist_ddot(v, w);
            const float vn = sqrtf(dot(v, v));
            if (vn > 0.0f) lower = fmaxf(lower, (float)vw / vn);
            bool stop = false;
            if (it > 0) {
                bool dup = false;
#pragma unroll
                for (int k = 0; k < 3; k++) dup = dup || (lam[k] > 0.0f && ia[k] == ja && ib[k] == jb);
                stop = dup || vv - vw <= (double)DIST_EPS * vv;
            }
            if (__builtin_amdgcn_readfirstlane(stop)) { status = 0; break; }
            // the nearest point of the features that hold w: weights l[0..2] of the slots and lw of w
            float l[3] = {0.0f, 0.0f, 0.0f}, lw = 1.0f;
            v3 nv = w;
            double nvv = dist_ddot(w, w);
#pragma unroll
            for (int k = 0; k < 3; k++) {                           // segments w -- slot k
                const v3 d = sr[k] - r;
                const float dd = dot(d, d);
                const float t = fminf(fmaxf(-dot(w, d) / dd, 0.0f), 1.0f);
                const v3 p = w + d * t;
                const double pp = dist_ddot(p, p);
                if (lam[k] > 0.0f && dd > 0.0f && pp < nvv) {
                    nvv = pp; nv = p; lw = 1.0f - t;
                    l[0] = l[1] = l[2] = 0.0f; l[k] = t;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {                           // triangles w, slot f, slot g: (0, 1), (1, 2), (2, 0)
                const int f = k, g = (k + 1) % 3;
                const v3 ab = sr[f] - r, ac = sr[g] - r, wf = sr[f] + cc, wg = sr[g] + cc;
                const float d1 = -dot(ab, w), d2 = -dot(ac, w), d3 = -dot(ab, wf), d4 = -dot(ac, wf), d5 = -dot(ab, wg), d6 = -dot(ac, wg);
                const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
                const v3 n = cross(ab, ac);
                const float nn = dot(n, n);
                const v3 p = n * (dot(n, w) / nn);
                const double pp = dist_ddot(p, p);
                const bool in = lam[f] > 0.0f && lam[g] > 0.0f && va > 0.0f && vb > 0.0f && vc > 0.0f && nn > 1e-10f * dot(ab, ab) * dot(ac, ac);
                if (in && pp < nvv) {
                    const float q = 1.0f / (va + vb + vc);
                    nvv = pp; nv = p; lw = va * q;
                    l[0] = l[1] = l[2] = 0.0f; l[f] = vb * q; l[g] = vc * q;
                }
            }
            bool inside = false;
            if (lam[0] > 0.0f && lam[1] > 0.0f && lam[2] > 0.0f) {  // the tetrahedron slot 0, 1, 2, w
                const v3 a = sr[0] + cc, ab = sr[1] - sr[0], ac = sr[2] - sr[0], ad = r - sr[0];
                const float V = dist_det(ab, ac, ad);
                const float La = dist_det(sr[1] + cc, sr[2] + cc, w), Lb = dist_det(a * -1.0f, ac, ad), Lc = dist_det(ab, a * -1.0f, ad), Ld = dist_det(ab, ac, a * -1.0f);
                const float sg = V > 0.0f ? 1.0f : -1.0f;
                inside = fabsf(V) > 1e-6f * sqrtf(dot(ab, ab) * dot(ac, ac) * dot(ad, ad)) && La * sg >= 0.0f && Lb * sg >= 0.0f && Lc * sg >= 0.0f && Ld * sg >= 0.0f;
            }
            if (__builtin_amdgcn_readfirstlane(inside)) { status = 1; tet = true; tr = r; tja = ja; tjb = jb; break; }
            if (__builtin_amdgcn_readfirstlane(it > 0 && !(nvv < vv))) { status = 0; break; }     // not strictly nearer: v stays
            // w into the first free slot
            bool placed = false;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const bool here = !placed && !(l[k] > 0.0f);
                if (here) { sr[k] = r; sA[k] = wa; sB[k] = wb; ia[k] = ja; ib[k] = jb; }
                lam[k] = here ? lw : l[k];
                placed = placed || here;
            }
            v = nv; vv = nvv;
            if (__builtin_amdgcn_readfirstlane(vv <= (double)DIST_TOUCH * DIST_TOUCH)) { status = 1; break; }
        }
        if (status == 1 && __builtin_amdgcn_readfirstlane(tet)) {
            // d.  The polytope's vertices, lane s holds slot s; the four faces of the tetrahedron in lanes 0..3, face f opposite vertex f.
            v3 pr = lane == 0 ? sr[0] : (lane == 1 ? sr[1] : (lane == 2 ? sr[2] : tr));
            int pia = lane == 0 ? ia[0] : (lane == 1 ? ia[1] : (lane == 2 ? ia[2] : tja));
            int pib = lane == 0 ? ib[0] : (lane == 1 ? ib[1] : (lane == 2 ? ib[2] : tjb));
            int nvert = 4;
            int f0 = lane == 0 ? 1 : 0, f1 = lane <= 1 ? 2 : 1, f2 = lane <= 2 ? 3 : 2;
            v3 fn; float fd;
            {
                const v3 A = lane == 0 ? sr[1] : sr[0], B = lane <= 1 ? sr[2] : sr[1], C = lane <= 2 ? tr : sr[2];
                const bool flip = dot(cross(B - A, C - A), pr - A) > 0.0f;      // the opposite vertex lies behind an outward face
                const int g = f1;
                f1 = flip ? f2 : f1; f2 = flip ? g : f2;
                sd_face(A, flip ? C : B, flip ? B : C, cc, &fn, &fd);
            }
            bool live = lane < 4;
            float best_up = INFINITY;
            v3 best_n = mk(0.0f, 0.0f, 0.0f);
            int F = 0;
            v3 nF = mk(0.0f, 0.0f, 0.0f);
            float dF = 0.0f, nw = 0.0f;
            status = 5;
            for (int t = 0; t < SD_TRIP_CAP; t++) {
                trips = t + 1;
                F = sd_nearest(live, fd, lane);
                nF = sd_lane(fn, F); dF = sd_lane(fd, F);
                if (__builtin_amdgcn_readfirstlane(!(dF < INFINITY))) { status = t == 0 ? 4 : 5; break; }         // no face with a normal: too flat to expand
                const int ja = dist_support(xa, nF, lane), jb = dist_support(xb, nF * -1.0f, lane);
                const v3 wa = dist_fetch(xa[0], xa[1], xa[2], ja), wb = dist_fetch(xb[0], xb[1], xb[2], jb);
                const v3 r = wa - wb;
                nw = sd_plane(nF, r, cc);
                if (nw < best_up) { best_up = nw; best_n = nF; }
                const bool dup = __ballot(lane < nvert && pia == ja && pib == jb) != 0ull;
                if (__builtin_amdgcn_readfirstlane(dup || nw - dF <= SD_EPS)) { status = 1; break; }
                // the visible faces, and of their directed edges (f0, f1), (f1, f2), (f2, f0) those whose reverse no visible face has
                const bool vis = live && (lane == F || sd_plane(fn, r, cc) - fd > 0.0f);
                const unsigned long long vmask = __ballot(vis), lmask = __ballot(live) & ~vmask;
                bool h0 = vis, h1 = vis, h2 = vis;
                for (unsigned long long m = vmask; m; m &= m - 1) {
                    const int l = __builtin_ctzll(m);
                    const int g0 = sd_slot(f0, l), g1 = sd_slot(f1, l), g2 = sd_slot(f2, l);
                    h0 = h0 && !((f0 == g1 && f1 == g0) || (f0 == g2 && f1 == g1) || (f0 == g0 && f1 == g2));
                    h1 = h1 && !((f1 == g1 && f2 == g0) || (f1 == g2 && f2 == g1) || (f1 == g0 && f2 == g2));
                    h2 = h2 && !((f2 == g1 && f0 == g0) || (f2 == g2 && f0 == g1) || (f2 == g0 && f0 == g2));
                }
                const unsigned long long b0 = __ballot(h0), b1 = __ballot(h1), b2 = __ballot(h2);
                if (__popcll(lmask) + __popcll(b0) + __popcll(b1) + __popcll(b2) > 64) break;      // the face cap: status 5
                // w is vertex nvert; each horizon edge (p, q), by edge number and then lane, takes the lowest free lane for the face (p, q, w)
                if (lane == nvert) { pr = r; pia = ja; pib = jb; }
                unsigned long long freem = ~lmask;
                bool fresh = false;
                int n0 = 0, n1 = 0;
                v3 A = mk(0.0f, 0.0f, 0.0f), B = A;
#pragma unroll
                for (int e = 0; e < 3; e++) {
                    for (unsigned long long m = e == 0 ? b0 : (e == 1 ? b1 : b2); m; m &= m - 1) {
                        const int l = __builtin_ctzll(m);
                        const int p = sd_slot(e == 0 ? f0 : (e == 1 ? f1 : f2), l), q = sd_slot(e == 0 ? f1 : (e == 1 ? f2 : f0), l);
                        const int tgt = __builtin_ctzll(freem) & 63;
                        freem &= freem - 1;
                        const v3 rp = sd_lane(pr, p), rq = sd_lane(pr, q);
                        if (lane == tgt) { n0 = p; n1 = q; A = rp; B = rq; fresh = true; }
                    }
                }
                if (fresh) {
                    f0 = n0; f1 = n1; f2 = nvert;
                    sd_face(A, B, r, cc, &fn, &fd);
                }
                live = (live && !vis) || fresh;
                nvert++;
            }
            if (status == 5 && trips == SD_TRIP_CAP) {                 // behind the last trip the nearest face is another one
                F = sd_nearest(live, fd, lane);
                nF = sd_lane(fn, F); dF = sd_lane(fd, F);
            }
            if (status == 4) {
                v3 xA = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int k = 0; k < 3; k++) xA = xA + sA[k] * lam[k];
                xA = xA + ca;
                o0 = make_float4(0.0f, 0.0f, xA.x, xA.y); o1 = make_float4(xA.z, xA.x, xA.y, xA.z); o2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {
                // the witness points: the origin's projection on face F in barycentric weights (float64), on the shapes' support vertices
                // Every lane weighs its own face; coplanar faces are the rule (table, shelf, cube faces), and among the faces in F's plane (a
                // distance within SD_EPS of d_F) the lowest lane whose triangle holds the projection gives the points, else F with clamped weights.
                const v3 r0 = mk(__shfl(pr.x, f0 & 63), __shfl(pr.y, f0 & 63), __shfl(pr.z, f0 & 63)), r1 = mk(__shfl(pr.x, f1 & 63), __shfl(pr.y, f1 & 63), __shfl(pr.z, f1 & 63)),
                         r2 = mk(__shfl(pr.x, f2 & 63), __shfl(pr.y, f2 & 63), __shfl(pr.z, f2 & 63));
                const v3 ab = r1 - r0, ac = r2 - r0;
                const double abc = dist_ddot(ab, cc), acc = dist_ddot(ac, cc);
                const double d1 = -(dist_ddot(ab, r0) + abc), d2 = -(dist_ddot(ac, r0) + acc), d3 = -(dist_ddot(ab, r1) + abc), d4 = -(dist_ddot(ac, r1) + acc),
                             d5 = -(dist_ddot(ab, r2) + abc), d6 = -(dist_ddot(ac, r2) + acc);
                const double ua = d3 * d6 - d5 * d4, ub = d5 * d2 - d1 * d6, uc = d1 * d4 - d3 * d2;
                const double us = ua + ub + uc;
                const bool holds = live && fd - dF <= SD_EPS && us > 0.0 && ua >= -1e-6 * us && ub >= -1e-6 * us && uc >= -1e-6 * us;
                const unsigned long long hmask = __ballot(holds);
                const int W = hmask ? (__builtin_ctzll(hmask) & 63) : F;
                const double va = fmax(ua, 0.0), vb = fmax(ub, 0.0), vc = fmax(uc, 0.0);
                const double sum = va + vb + vc;
                const bool okw = sum > 0.0;
                const float m0 = okw ? (float)(va / sum) : 1.0f, m1 = okw ? (float)(vb / sum) : 0.0f, m2 = okw ? (float)(vc / sum) : 0.0f;
                const float l0 = sd_lane(m0, W), l1 = sd_lane(m1, W), l2 = sd_lane(m2, W);
                const int g0 = sd_slot(f0, W), g1 = sd_slot(f1, W), g2 = sd_slot(f2, W);
                const int a0 = min(max(__builtin_amdgcn_readlane(pia, g0), 0), 64 * DIST_TRIPS - 1), a1 = min(max(__builtin_amdgcn_readlane(pia, g1), 0), 64 * DIST_TRIPS - 1),
                          a2 = min(max(__builtin_amdgcn_readlane(pia, g2), 0), 64 * DIST_TRIPS - 1);
                const int c0 = min(max(__builtin_amdgcn_readlane(pib, g0), 0), 64 * DIST_TRIPS - 1), c1 = min(max(__builtin_amdgcn_readlane(pib, g1), 0), 64 * DIST_TRIPS - 1),
                          c2 = min(max(__builtin_amdgcn_readlane(pib, g2), 0), 64 * DIST_TRIPS - 1);
                const v3 xA = dist_fetch(xa[0], xa[1], xa[2], a0) * l0 + dist_fetch(xa[0], xa[1], xa[2], a1) * l1 + dist_fetch(xa[0], xa[1], xa[2], a2) * l2 + ca;
                const v3 xB = dist_fetch(xb[0], xb[1], xb[2], c0) * l0 + dist_fetch(xb[0], xb[1], xb[2], c1) * l1 + dist_fetch(xb[0], xb[1], xb[2], c2) * l2 + cb;
                // status 1: the final face's own width n . w; status 5: the smallest width seen, with its direction
                const float up = status == 1 ? nw : best_up;
                const v3 n = (status == 1 ? nF : best_n) * -1.0f;
                o0 = make_float4(-up, -dF, xA.x, xA.y); o1 = make_float4(xA.z, xB.x, xB.y, xB.z); o2 = make_float4(n.x, n.y, n.z, 0.0f);
            }
        } else {
            v3 xA = mk(0.0f, 0.0f, 0.0f), xB = xA;                  // the weighted vertices about the centres, then the centres
#pragma unroll
            for (int k = 0; k < 3; k++) { xA = xA + sA[k] * lam[k]; xB = xB + sB[k] * lam[k]; }
            xA = xA + ca; xB = xB + cb;
            if (status == 1) {
                status = 4;                                         // touching: today's overlap row
                o0 = make_float4(0.0f, 0.0f, xA.x, xA.y); o1 = make_float4(xA.z, xA.x, xA.y, xA.z); o2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {
                const float dist = sqrtf((float)vv);
                const v3 n = v * (1.0f / dist);
                o0 = make_float4(dist, fminf(lower, dist), xA.x, xA.y); o1 = make_float4(xA.z, xB.x, xB.y, xB.z); o2 = make_float4(n.x, n.y, n.z, 0.0f);
            }
        }
    }
    SdItem R;
    R.o0 = o0; R.o1 = o1; R.o2 = o2; R.status = status; R.iters = iters; R.trips = trips; R.ota = ota; R.oia = oia; R.otb = otb; R.oib = oib;
    return R;
}

template <bool CARRY>
__global__ void __launch_bounds__(SD_THREADS) k_signed_distance(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                const float *__restrict__ postures /*[N][K][11] or null: the present state, K = 1*/, int K,
                                                                float4 *__restrict__ out_deep /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                float *__restrict__ out_signed /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/,
                                                                float4 *__restrict__ out_pts /*[N][Q][3] or null*/,
                                                                const float *__restrict__ att /*[N][NOBJ][ATT_ROW]; null and unread without CARRY*/) {
    static_assert(RAY_ST == 32 && NB == 11 && ST_OPOS == 2 * NB, "staged slot s is joint s (s < 11) or state slot s + 11");
    static_assert(64 * DIST_TRIPS == VMAXC && 4 + SD_TRIP_CAP <= 64, "a lane holds three vertices of a shape and one of the polytope");
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][RAY_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    __shared__ float s_best[SD_WAVES][SD_PARK];
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row = blockIdx.x;                                    // e * K + k
    const int env = min((int)(row / (size_t)K), N - 1);
    // 1
    if (tid < RAY_ST) s_st[tid][0] = tid < NB ? (postures ? postures[row * NB + tid] : D.state[(size_t)tid * N + env]) : D.state[(size_t)(tid + NB) * N + env];
    __syncthreads();
    // 2
    if (tid == 0) {
        float *fr = s_fr[0];
        for (int b = 0; b < NB; b++) {
            const int p = PARENT[b];
            m3 Rp = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
            v3 pp = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]);
            if (p >= 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) Rp.m[k] = fr[9 * p + k];
                pp = mk(fr[RAY_FR_P + 3 * p], fr[RAY_FR_P + 3 * p + 1], fr[RAY_FR_P + 3 * p + 2]);
            }
            m3 jr;
#pragma unroll
            for (int k = 0; k < 9; k++) jr.m[k] = B.jrot[b][k];
            const m3 Rj = nc::mul(Rp, jr);
            const v3 ax = mk(B.axis[b][0], B.axis[b][1], B.axis[b][2]);
            const v3 pb = nc::add(pp, nc::mulv(Rp, mk(B.jpos[b][0], B.jpos[b][1], B.jpos[b][2])));
            const m3 Rb = nc::mul(Rj, nc::axis_angle(ax, s_st[ST_Q + b][0]));
#pragma unroll
            for (int k = 0; k < 9; k++) fr[9 * b + k] = Rb.m[k];
            fr[RAY_FR_P + 3 * b] = pb.x; fr[RAY_FR_P + 3 * b + 1] = pb.y; fr[RAY_FR_P + 3 * b + 2] = pb.z;
        }
    } else if (!CARRY && tid < 1 + NOBJ) {
        const int o = tid - 1;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][0], s_st[21 + 4 * o][0], s_st[22 + 4 * o][0], s_st[23 + 4 * o][0]);
        float *ob = s_ob[0] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][0]; ob[10] = s_st[12 + 3 * o][0]; ob[11] = s_st[13 + 3 * o][0];
    }
    __syncthreads();
    if constexpr (CARRY) {
        if (tid >= 1 && tid < 1 + NOBJ) carry_stage_object(att, env, tid - 1, s_st, s_fr[0], s_ob[0]);
        __syncthreads();
    }
    // 3
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    float key = INFINITY;
    int bj = wave, bst = 0, ba = -1, bb = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0, b2 = b0;
    for (int j = wave; j < Q; j += SD_WAVES) {
        const SdItem R = sd_pair(S, tab, j, s_fr[0], s_ob[0], cull, maxd, lane);
        if (lane == 0) {
            out_signed[row * Q + j] = R.o0.x;
            out_status[row * Q + j] = (R.status & 255) | ((R.iters & 255) << 8) | ((R.trips & 255) << 16);
            if (out_pts) { out_pts[3 * (row * Q + j)] = R.o0; out_pts[3 * (row * Q + j) + 1] = R.o1; out_pts[3 * (row * Q + j) + 2] = R.o2; }
        }
        const float d = pc_uniform(R.o0.x);
        const bool nearer = d < key;
        if (nearer || j == wave) {                                      // (uniform in the wave)
            bj = j; bst = __builtin_amdgcn_readfirstlane(R.status);
            ba = __builtin_amdgcn_readfirstlane(R.ota == 0 ? -1 : (R.ota == 1 ? R.oia : 16 + R.oia));
            bb = __builtin_amdgcn_readfirstlane(R.otb == 0 ? -1 : (R.otb == 1 ? R.oib : 16 + R.oib));
            b0 = pc_uniform(R.o0); b1 = pc_uniform(R.o1); b2 = pc_uniform(R.o2);
        }
        key = nearer ? d : key;
    }
    // 4
    if (lane == 0) {
        float *w = s_best[wave];
        w[0] = b0.x; w[1] = b0.y; w[2] = b0.z; w[3] = b0.w; w[4] = b1.x; w[5] = b1.y; w[6] = b1.z; w[7] = b1.w;
        w[8] = b2.x; w[9] = b2.y; w[10] = b2.z; w[11] = b2.w;
        w[12] = key; w[13] = __int_as_float(bj); w[14] = __int_as_float(bst); w[15] = __int_as_float(ba); w[16] = __int_as_float(bb);
    }
    __syncthreads();
    if (tid == 0) {
        int win = 0;
        for (int w = 1; w < SD_WAVES; w++) {
            const bool lower = s_best[w][12] < s_best[win][12] ||
                               (s_best[w][12] == s_best[win][12] && __float_as_int(s_best[w][13]) < __float_as_int(s_best[win][13]));
            win = (w < Q && lower) ? w : win;                               // a wave behind the table's end had no pair
        }
        const float *w = s_best[win];
        out_deep[3 * row] = make_float4(w[0], w[1], w[2], w[3]);
        out_deep[3 * row + 1] = make_float4(w[4], w[5], w[6], w[7]);
        out_deep[3 * row + 2] = make_float4(w[8], w[9], w[10], w[11]);
        out_id[row] = make_int4(__float_as_int(w[14]), __float_as_int(w[13]), __float_as_int(w[15]), __float_as_int(w[16]));
    }
}
