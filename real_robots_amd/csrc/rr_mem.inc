// rr_mem.inc -- the one owner of every block of memory that belongs to an rr_env, and the one way to get more (host only, no HIP type):
// device and pinned host blocks, rr_create's and those a feature allocates on first use.  A caller hands acquire() a list of parts --
// the address of the handle's pointer, the bytes, zero-filled or not, the kind -- and gets ALL of them or NOTHING: on a failed
// allocation or fill the list's blocks are freed again, no pointer of the list has changed, the owner is as before, and the backend's
// error text comes back for the caller's fail(RR_EDEVICE, "<entry point>: allocating <what>: ...").  A block is owned from the
// moment it exists (before it is filled).  The four primitives come in as function pointers: rr_host.inc has the HIP ones,
// tests/test_mem_owner.py compiles this file alone with a fake that fails the k-th allocation or fill.
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <vector>

enum MemKind { MEM_DEVICE, MEM_PINNED, MEM_PINNED_MAPPED };   // device | pinned host | pinned host, mapped into the device's address space
#define MEM_SLACK 16         // bytes behind every device part (allocated and, where asked, zero-filled with it)
struct MemBackend {
    void *ctx;
    void *(*alloc)(void *ctx, MemKind kind, size_t bytes, const char **err);   // nullptr and *err on failure
    const char *(*zero)(void *ctx, void *dev, size_t bytes);                   // zero-fill of device memory; nullptr or the error
    void (*release)(void *ctx, MemKind kind, void *p);
};
struct MemPart { void **ptr; size_t bytes; bool zero; MemKind kind; };
template <typename T>
static inline MemPart mem_part(T **ptr, size_t bytes, bool zero = true, MemKind kind = MEM_DEVICE) { return MemPart{(void **)ptr, bytes, zero, kind}; }

struct MemOwner {
    struct Block { void *p; MemKind kind; };
    MemBackend be = {};
    std::vector<Block> blocks;
    void drop_from(size_t n) { while (blocks.size() > n) { be.release(be.ctx, blocks.back().kind, blocks.back().p); blocks.pop_back(); } }
    // all parts or none; nullptr or the backend's error text.  (A pinned part is zero-filled here: host memory, nothing to fail.)
    const char *acquire(const MemPart *parts, size_t n) {
        const size_t before = blocks.size();
        blocks.reserve(before + n);
        const char *err = nullptr;
        for (size_t i = 0; i < n && !err; i++) {
            const MemPart &t = parts[i];
            const size_t bytes = t.bytes + (t.kind == MEM_DEVICE ? MEM_SLACK : 0);
            void *p = be.alloc(be.ctx, t.kind, bytes, &err);
            if (!p) { if (!err) err = "allocation failed"; break; }
            blocks.push_back(Block{p, t.kind});
            if (t.zero && t.kind == MEM_DEVICE) err = be.zero(be.ctx, p, bytes);
            else if (t.zero) memset(p, 0, bytes);
        }
        if (err) { drop_from(before); return err; }
        for (size_t i = 0; i < n; i++) *parts[i].ptr = blocks[before + i].p;
        return nullptr;
    }
    const char *acquire(std::initializer_list<MemPart> parts) { return acquire(parts.begin(), parts.size()); }
    // one block back (the replaceable ones): freed once and forgotten, the caller's pointer cleared; a null or unknown pointer: nothing freed
    template <typename T>
    void release(T *&p) {
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i].p == (const void *)p) { be.release(be.ctx, blocks[i].kind, blocks[i].p); blocks.erase(blocks.begin() + (std::ptrdiff_t)i); break; }
        p = nullptr;
    }
    void release_all() { drop_from(0); }      // rr_destroy's single call for memory
};
