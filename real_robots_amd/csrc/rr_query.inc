// rr_query.inc -- the output buffers of the whole-batch query families (host only, no HIP type): ONE table that says how many bytes
// every buffer of every family has, and ONE pair of accessors behind the twenty rr_*_buffer / rr_*_copy_to_host entry points.  What
// needs the handle or the device comes in as a small view and three function pointers, the way MemOwner takes its MemBackend:
// rr_host.inc has the HIP ones, tests/test_query_layout.py compiles this file alone with a fake that counts.
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/realrobot.h"

enum { QRY_JOINTS = 11, QRY_LINKS = 17 };    // the model's constants, once: the joints of q[11], the URDF links of rr_link_poses
// What a buffer's size depends on: envs N, rows K (postures, segments or targets per env), pairs Q, points or rays P, objects.
enum { QD_N, QD_K, QD_Q, QD_P, QD_OBJECTS, QD_COUNT };
struct QueryDims { size_t d[QD_COUNT]; };
#define QB(dim) (1u << QD_##dim)
// One buffer: `unit` bytes times every dimension of `over`.
struct QueryBuffer { size_t unit; unsigned over; };
enum { QF_KIN, QF_RAY, QF_DIST, QF_PC, QF_SD, QF_SG, QF_SW, QF_PK, QF_PIK, QF_PD, QF_COUNT };
#define QUERY_MAX_BUFFERS 7
// One family: its entry points are <stem>_buffer and <stem>_copy_to_host, `which` is in [0, count), and its group is allocated
// once for RR_PC_MAX_POSTURES rows of RR_DIST_MAX pairs and `max_p` points or rays.
struct QueryFamily { const char *stem, *count_name; int count; size_t max_p; QueryBuffer buf[QUERY_MAX_BUFFERS]; };
static const QueryFamily QUERY_FAMILIES[QF_COUNT] = {
    {"rr_kinematic", "RR_KIN_COUNT", RR_KIN_COUNT, RR_KIN_MAX_POINTS,
     {{QRY_JOINTS * 4, QB(N)}, {QRY_LINKS * 7 * 4, QB(N)}, {QRY_LINKS * 6 * 4, QB(N)}, {6 * 4, QB(N) | QB(OBJECTS)},
      {3 * 4, QB(N) | QB(P)}, {6 * 4, QB(N) | QB(P)}, {6 * QRY_JOINTS * 4, QB(N) | QB(P)}}},
    {"rr_ray", "RR_RAY_COUNT", RR_RAY_COUNT, RR_RAY_MAX, {{32, QB(N) | QB(P)}, {16, QB(N) | QB(P)}}},
    {"rr_distance", "RR_DIST_COUNT", RR_DIST_COUNT, 0, {{48, QB(N) | QB(Q)}, {16, QB(N) | QB(Q)}}},
    {"rr_posture", "RR_PC_COUNT", RR_PC_COUNT, 0, {{48, QB(N) | QB(K)}, {16, QB(N) | QB(K)}, {4, QB(N) | QB(K) | QB(Q)}, {4, QB(N) | QB(K) | QB(Q)}}},
    {"rr_signed", "RR_SD_COUNT", RR_SD_COUNT, 0,
     {{48, QB(N) | QB(K)}, {16, QB(N) | QB(K)}, {4, QB(N) | QB(K) | QB(Q)}, {4, QB(N) | QB(K) | QB(Q)}, {48, QB(N) | QB(Q)}}},
    {"rr_signed_gradient", "RR_SG_COUNT", RR_SG_COUNT, 0, {{48, QB(N) | QB(K)}, {48, QB(N) | QB(K)}, {48, QB(N) | QB(Q)}}},
    {"rr_sweep", "RR_SW_COUNT", RR_SW_COUNT, 0, {{48, QB(N) | QB(K)}, {48, QB(N) | QB(K)}, {16, QB(N) | QB(K)}, {4, QB(N) | QB(K) | QB(Q)}}},
    {"rr_posture_kinematics", "RR_PK_COUNT", RR_PK_COUNT, RR_KIN_MAX_POINTS,
     {{QRY_LINKS * 7 * 4, QB(N) | QB(K)}, {3 * 4, QB(N) | QB(K) | QB(P)}, {6 * QRY_JOINTS * 4, QB(N) | QB(K) | QB(P)}}},
    {"rr_posture_ik", "RR_PIK_COUNT", RR_PIK_COUNT, 0, {{QRY_JOINTS * 4, QB(N) | QB(K)}, {4 * 4, QB(N) | QB(K)}, {2 * 4, QB(N) | QB(K)}}},
    {"rr_posture_dynamics", "RR_PD_COUNT", RR_PD_COUNT, 0,
     {{QRY_JOINTS * QRY_JOINTS * 4, QB(N) | QB(K)}, {QRY_JOINTS * 4, QB(N) | QB(K)}, {QRY_JOINTS * 4, QB(N) | QB(K)}, {QRY_JOINTS * 4, QB(N) | QB(K)},
      {QRY_JOINTS * QRY_JOINTS * 4, QB(N) | QB(K)}}},
};
#undef QB

static inline size_t query_bytes(int family, int which, const QueryDims &dims) {
    const QueryBuffer &b = QUERY_FAMILIES[family].buf[which];
    size_t n = b.unit;
    for (int k = 0; k < QD_COUNT; k++)
        if ((b.over >> k) & 1u) n *= dims.d[k];
    return n;
}
// the dimensions a family's group is allocated for
static inline QueryDims query_capacity(int family, size_t N, size_t objects) {
    return QueryDims{{N, RR_PC_MAX_POSTURES, RR_DIST_MAX, QUERY_FAMILIES[family].max_p, objects}};
}

// What the accessors need from a handle: the family, its array of buffer pointers (read behind `ensure`, which may fill it) and the
// layout in force.  env == nullptr: the caller's handle was null.
struct QueryView { void *env; int family; void *const *buf; QueryDims dims; };
struct QueryBackend {
    int (*ensure)(void *env, int family, const char *who);                    // the family's buffers exist afterwards: RR_OK, or the code of a refusal it has reported
    int (*copy)(void *env, void *dst, const void *src, size_t bytes);         // device to host on the handle's stream, and the wait; RR_OK or a reported code
    int (*fail)(int code, const std::string &msg);                            // the error sink: keeps the text, returns the code
};

static inline int query_bad_which(const QueryFamily &f, const QueryBackend &be, const std::string &who, int32_t which) {
    return be.fail(RR_EINVAL, who + ": buffer " + std::to_string(which) + " is not in [0, " + f.count_name + ")");
}

// <stem>_buffer: device pointer and bytes in force of buffer `which`; a refused call touches neither output
static int query_buffer(const QueryView &v, const QueryBackend &be, int32_t which, void **dev_ptr, size_t *bytes) {
    const QueryFamily &f = QUERY_FAMILIES[v.family];
    const std::string who = std::string(f.stem) + "_buffer";
    if (!v.env) return be.fail(RR_EINVAL, who + ": null env");
    if (which < 0 || which >= f.count) return query_bad_which(f, be, who, which);
    const int rc = be.ensure(v.env, v.family, who.c_str());
    if (rc != RR_OK) return rc;
    if (dev_ptr) *dev_ptr = v.buf[which];
    if (bytes) *bytes = query_bytes(v.family, which, v.dims);
    return RR_OK;
}

// <stem>_copy_to_host: buffer `which` to host memory of exactly its bytes in force (none: nothing to copy)
static int query_copy_to_host(const QueryView &v, const QueryBackend &be, int32_t which, void *dst, size_t bytes) {
    const QueryFamily &f = QUERY_FAMILIES[v.family];
    const std::string who = std::string(f.stem) + "_copy_to_host";
    if (!v.env) return be.fail(RR_EINVAL, who + ": null env");
    if (!dst) return be.fail(RR_EINVAL, who + ": null destination");
    if (which < 0 || which >= f.count) return query_bad_which(f, be, who, which);
    if (bytes != query_bytes(v.family, which, v.dims)) return be.fail(RR_EINVAL, who + ": size mismatch");
    const int rc = be.ensure(v.env, v.family, who.c_str());
    if (rc != RR_OK) return rc;
    return bytes ? be.copy(v.env, dst, v.buf[which], bytes) : RR_OK;
}
