// rr_fork.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_fork: env records gathered on the device (rr_copy_envs, realrobot.h): the record of env i of the destination becomes the
// record of env idx[i] of the source -- between the running envs (a fork), from them into a snapshot slot (save), back (restore,
// or one saved env into many running ones), or from slot to slot.  A record is what a checkpoint carries for an env minus its
// settings (ckpt_copy in rr_host.inc): the state slab with the motor targets, the contact list of the last solved step with its
// normal forces -- the history of the warm start --, the clocks, the error flags, the touch sensors and the published count /
// class.  Launched by rr_snapshot_slots / rr_copy_envs alone, never by a step.
//
// A plain gather, bound by memory traffic; no LDS, no atomics, ordinary vector loads and stores.  The envs go in groups of
// FK_GROUP = 64 consecutive DESTINATION envs, five 256-thread workgroups to a group (blockIdx.y):
//   y == 0      the SoA part.  The state slab is [72][N]: lane l of every wave is env 64 g + l, so each of a wave's stores is
//               one 256-byte line; the four waves take the rows r = w, w + 4, ... (18 each, all loads issued before the first
//               store).  The index maps that matter read just as well: the identity reads the same lines, a broadcast one word
//               per row.  Behind the slab the waves share the six per-env arrays (four 4-byte words and the float4 of the
//               touch sensors per env).
//   y == 1 .. 4 the contact lists of sixteen envs of the group each, sixteen lanes to an env: an env's list is 2 304 contiguous
//               bytes of which the rows below min(count, MAXC) are live -- 3 count float4 rows and ceil(count / 4) float4 of
//               forces, 16-byte accesses, a quarter wave reading 256 contiguous bytes per pass.  Rows from the count on are NOT
//               copied: every reader of the list stops at the count (k_collide's warm-start matching, k_solve, k_contact_obs,
//               rr_get_contacts), so in a destination they are unspecified.
// The list part reads the count from the SOURCE, as the SoA part does: neither waits for the other.
// An index outside [0, N) -- -1 by contract, anything else in a device index -- keeps the destination env as it is; the test
// comes before any address is formed from the index.  `identity`: the second launch of a staged in-place copy, env i from
// env i of the staging slot for exactly the envs whose index is valid (rr_copy_envs).
// Source and destination are never the same arrays with a non-identity map: rr_copy_envs stages those copies.
#define FK_GROUP 64
#define FK_ROWS (ST_TOTAL / 4)     // state rows per wave of the SoA workgroup

// One set of records: the running envs (DevPtrs' arrays of the frame of the last solved step) or a snapshot slot.
struct ForkRec {
    float *state;        // [ST_TOTAL][N]
    int *ccount;         // [N]
    float4 *clist;       // [N][MAXC][3]
    float *cforce;       // [N][MAXC]
    int *timestep;       // [N]
    unsigned *errflags;  // [N]
    float *touch;        // [N][4]
    int *ccount_pub, *class_pub;   // [N]
};

// source env of destination env i, or -1: keep
__device__ __forceinline__ int fork_source(const int *idx, int identity, int N, int i) {
    if (!idx) return i;
    const int s = idx[i];
    if ((unsigned)s >= (unsigned)N) return -1;
    return identity ? i : s;
}

// err_mask: the error bits a destination takes over (all of them into a slot; 1 | 2 | 4 into a running env, whose bit 8 -- the
// status of its own last rendered frame -- is cleared, as rr_set_state does)
__global__ void __launch_bounds__(256) k_fork(int N, ForkRec src, ForkRec dst, const int *__restrict__ idx, int identity, unsigned err_mask) {
    static_assert(ST_TOTAL % 4 == 0, "the state rows are dealt out evenly among four waves");
    static_assert(MAXC % 4 == 0 && MAXC / 4 <= 16, "an env's forces are at most one float4 per lane of its sixteen");
    const int tid = threadIdx.x;
    if (blockIdx.y == 0) {
        const int w = tid >> 6, i = blockIdx.x * FK_GROUP + (tid & 63);
        if (i >= N) return;
        const int s = fork_source(idx, identity, N, i);
        if (s < 0) return;
        float v[FK_ROWS];
#pragma unroll
        for (int k = 0; k < FK_ROWS; k++) v[k] = src.state[(size_t)(w + 4 * k) * N + s];
#pragma unroll
        for (int k = 0; k < FK_ROWS; k++) dst.state[(size_t)(w + 4 * k) * N + i] = v[k];
        if (w == 0) { dst.ccount[i] = src.ccount[s]; dst.timestep[i] = src.timestep[s]; }
        else if (w == 1) { dst.errflags[i] = src.errflags[s] & err_mask; dst.ccount_pub[i] = src.ccount_pub[s]; }
        else if (w == 2) dst.class_pub[i] = src.class_pub[s];
        else ((float4 *)dst.touch)[i] = ((const float4 *)src.touch)[s];
        return;
    }
    const int i = blockIdx.x * FK_GROUP + ((int)blockIdx.y - 1) * 16 + (tid >> 4), l = tid & 15;
    if (i >= N) return;
    const int s = fork_source(idx, identity, N, i);
    if (s < 0) return;
    const int count = max(0, min(src.ccount[s], MAXC));
    const float4 *sl = src.clist + (size_t)s * MAXC * 3;
    float4 *dl = dst.clist + (size_t)i * MAXC * 3;
    for (int u = l; u < 3 * count; u += 16) dl[u] = sl[u];
    if (4 * l < count) ((float4 *)(dst.cforce + (size_t)i * MAXC))[l] = ((const float4 *)(src.cforce + (size_t)s * MAXC))[l];
}
