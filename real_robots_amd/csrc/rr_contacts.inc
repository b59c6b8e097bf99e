// rr_contacts.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_contact_obs: the contact list of the last solved step as whole-batch observations (rr_contact_observations, realrobot.h):
// Kuka.get_contacts (robot.py:131-150) for every env at once -- one 12-float record per contact, and per body {max, sum} of
// the normal force with a mask of what the body touches.  Read-only on the simulation; launched by rr_contact_observations
// alone, never by a step.
//
// One wave per env, four envs per 256-thread workgroup (2.5 KB in, 2.5 KB out per env: memory-bound, no reuse between envs).
// Lanes 0..47 take one contact slot each: three 16-byte loads of the device record {x y z nx | ny nz dist meta | mu ...}, the
// force, three 16-byte stores of the row rr_get_contacts makes on the host -- all-zero rows from the env's count on -- and a
// stash of {row of body A, row of body B, partner bits, force} in the wave's LDS region.  Lanes 0..RR_CONTACT_ROWS-1 then walk
// the stash in ASCENDING contact index, each for its own row: plain float32 compares and adds, one after the other, from 0.0f
// (every lane reads the same LDS word: a broadcast).  No lane-tree reduction: the sums are those of a sequential float32 loop
// in contact order, bit for bit (tests/numpy_contacts.py).
//
// Rows: 0 .. nl-1 the robot's URDF links (a contact whose body A is a robot body, 0..15, goes to the row of its linkA),
// nl + i object i (body 16 + i, as A or as B).  Only contacts with |distance| < 0.1f count (robot.py:136; the solve's meta_near
// bit is not in the stored meta: it is computed again from the stored distance, the same compare on the same float).
// Partner bits of a row: 0 a static body (-1), 1 + j object j, 4 the robot.  The pair table (parse_model) has body A = robot
// or object and body B = static or object: NO pair has a robot body as B, so bit 4 only ever appears on object rows (the
// contact's B side) and a link row never has it; were such a pair added, its A row would get bit 4 by the same expression.
#define CO_ENVS 4            // envs (waves) per workgroup
#define CO_NONE 255          // stash: no row

__global__ void __launch_bounds__(64 * CO_ENVS) k_contact_obs(SimParams P, DevPtrs D, int nl, float4 *__restrict__ contacts /*[N][MAXC][3]*/,
                                                              float2 *__restrict__ body_force /*[N][RR_CONTACT_ROWS]*/, unsigned *__restrict__ body_partners /*[N][RR_CONTACT_ROWS]*/) {
    static_assert(MAXC <= 64 && RR_CONTACT_ROWS <= 64, "one lane per contact slot / per row");
    __shared__ unsigned s_key[CO_ENVS][MAXC];      // row A | row B << 8 | partner bits of A's row << 16 | of B's row << 24
    __shared__ float s_force[CO_ENVS][MAXC];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int env = blockIdx.x * CO_ENVS + w;
    const bool live = env < P.N;                   // (the barrier below is reached by every thread)
    int count = 0;
    if (live) {
        count = max(0, min(D.ccount[env], MAXC));
        if (lane < MAXC) {
            float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o1 = o0, o2 = o0;
            unsigned key = CO_NONE | (CO_NONE << 8);
            float f = 0.0f;
            if (lane < count) {
                const float4 *r = D.clist + ((size_t)env * MAXC + lane) * 3;
                const float4 r0 = r[0], r1 = r[1], r2 = r[2];
                f = D.cforce[(size_t)env * MAXC + lane];
                const int meta = __float_as_int(r1.w);
                const int bodyA = (signed char)(meta & 255), bodyB = (signed char)((meta >> 8) & 255), linkA = (signed char)((meta >> 16) & 255);
                o0 = make_float4((float)bodyA, (float)bodyB, (float)linkA, r0.x);
                o1 = make_float4(r0.y, r0.z, r0.w, r1.x);
                o2 = make_float4(r1.y, r1.z, f, r2.x);
                if (fabsf(r1.z) < 0.1f) {          // robot.py:136 contact_threshold
                    const bool a_robot = bodyA >= 0 && bodyA < 16;
                    const int ia = bodyA - 16, ib = bodyB - 16;
                    const unsigned rowA = a_robot ? ((linkA >= 0 && linkA < nl) ? (unsigned)linkA : CO_NONE) : ((ia >= 0 && ia < NOBJ) ? (unsigned)(nl + ia) : CO_NONE);
                    const unsigned rowB = (ib >= 0 && ib < NOBJ) ? (unsigned)(nl + ib) : CO_NONE;
                    const unsigned bitsA = bodyB < 0 ? 1u : (bodyB >= 16 ? 2u << min(ib, NOBJ - 1) : 16u);
                    const unsigned bitsB = a_robot ? 16u : 2u << max(0, min(ia, NOBJ - 1));
                    key = rowA | (rowB << 8) | (bitsA << 16) | (bitsB << 24);
                }
            }
            float4 *o = contacts + ((size_t)env * MAXC + lane) * 3;
            o[0] = o0; o[1] = o1; o[2] = o2;
            s_key[w][lane] = key;
            s_force[w][lane] = f;
        }
    }
    __syncthreads();
    if (live && lane < RR_CONTACT_ROWS) {
        float mx = 0.0f, sum = 0.0f;
        unsigned bits = 0u;
        for (int c = 0; c < count; c++) {
            const unsigned key = s_key[w][c];
            const float f = s_force[w][c];
            if ((key & 255u) == (unsigned)lane) { mx = f > mx ? f : mx; sum = sum + f; bits |= (key >> 16) & 255u; }
            if (((key >> 8) & 255u) == (unsigned)lane) { mx = f > mx ? f : mx; sum = sum + f; bits |= key >> 24; }
        }
        body_force[(size_t)env * RR_CONTACT_ROWS + lane] = make_float2(mx, sum);
        body_partners[(size_t)env * RR_CONTACT_ROWS + lane] = bits;
    }
}
