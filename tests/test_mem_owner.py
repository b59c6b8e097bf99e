"""The owner of a handle's memory (real_robots_amd/csrc/rr_mem.inc, MemOwner) -- checked on the CPU.  The file is compiled alone with
g++ (no HIP, no rr_env) into a driver with a fake backend: it counts the live blocks per kind, records every requested size and every
fill, aborts on a double free or on a free of a pointer it never handed out, and fails the k-th allocation or the k-th fill when told to.
A group of five mixed parts (device and pinned, zero-filled and not) is acquired on top of an owner that already holds two blocks, with
every allocation and every fill failing in turn: nothing may change, and the retry must get exactly what was asked for.  Built a second
time with -fsanitize=address,undefined (a stand-alone program: no sanitizer comes near code loaded into Python).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'real_robots_amd', 'csrc')

SLACK = 16
DEVICE, PINNED, MAPPED = 0, 1, 2
# (kind, bytes, zero-filled): the group under test
PARTS = [(DEVICE, 100, 1), (PINNED, 64, 0), (DEVICE, 1000, 0), (MAPPED, 48, 1), (DEVICE, 7, 1)]
N_ALLOCS = len(PARTS)
FILLED = [i for i, (kind, _, zero) in enumerate(PARTS) if kind == DEVICE and zero]      # the parts whose fill goes through the backend
REQUESTED = [nbytes + (SLACK if kind == DEVICE else 0) for kind, nbytes, _ in PARTS]

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <map>
#include "rr_mem.inc"

struct Fake {
    struct Live { MemKind kind; size_t bytes; };
    std::map<void *, Live> live;
    std::vector<size_t> sizes;                   // every requested size, in order
    std::vector<void *> fills; std::vector<size_t> fill_bytes;
    int allocs = 0, zeros = 0, frees = 0, fail_alloc = 0, fail_fill = 0;     // fail_*: 1-based index of the call that fails (0: none)
    int count(bool device) const { int n = 0; for (auto &kv : live) n += (kv.second.kind == MEM_DEVICE) == device; return n; }
};
static void *f_alloc(void *ctx, MemKind kind, size_t bytes, const char **err) {
    Fake *f = (Fake *)ctx;
    f->sizes.push_back(bytes);
    if (++f->allocs == f->fail_alloc) { *err = "fake: out of memory"; return nullptr; }
    void *p = malloc(bytes ? bytes : 1);
    memset(p, 0xab, bytes);
    f->live[p] = Fake::Live{kind, bytes};
    return p;
}
static const char *f_zero(void *ctx, void *p, size_t bytes) {
    Fake *f = (Fake *)ctx;
    if (++f->zeros == f->fail_fill) return "fake: fill failed";
    auto it = f->live.find(p);
    if (it == f->live.end() || it->second.kind != MEM_DEVICE || bytes > it->second.bytes) { fprintf(stderr, "fill of an unknown block\n"); abort(); }
    f->fills.push_back(p); f->fill_bytes.push_back(bytes);
    memset(p, 0, bytes);
    return nullptr;
}
static void f_release(void *ctx, MemKind kind, void *p) {
    Fake *f = (Fake *)ctx;
    auto it = f->live.find(p);
    if (it == f->live.end() || it->second.kind != kind) { fprintf(stderr, "double free / free of an unknown pointer\n"); abort(); }
    f->live.erase(it); f->frees++;
    free(p);
}
static bool same(const std::vector<MemOwner::Block> &a, const std::vector<MemOwner::Block> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].p != b[i].p || a[i].kind != b[i].kind) return false;
    return true;
}
static bool holds(const MemOwner &m, const void *p) { for (auto &b : m.blocks) if (b.p == p) return true; return false; }

// argv: fail_alloc fail_fill retry, then the parts as kind bytes zero ...
int main(int argc, char **argv) {
    Fake f;
    MemOwner m;
    m.be = MemBackend{&f, f_alloc, f_zero, f_release};
    // what the handle held before: a device and a pinned block
    float *old_dev = nullptr; char *old_pin = nullptr;
    if (m.acquire({mem_part(&old_dev, 40), mem_part(&old_pin, 24, false, MEM_PINNED)})) return 2;
    const int n = (argc - 4) / 3;
    const bool retry = atoi(argv[3]) != 0;
    std::vector<MemPart> parts((size_t)n);
    std::vector<void *> ptr((size_t)n), prev((size_t)n);
    for (int i = 0; i < n; i++) {
        prev[i] = ptr[i] = (void *)(size_t)(0x1000 + 8 * i);             // (never dereferenced: "the pointer's previous value")
        parts[i] = mem_part(&ptr[i], (size_t)atol(argv[5 + 3 * i]), atoi(argv[6 + 3 * i]) != 0, (MemKind)atoi(argv[4 + 3 * i]));
    }
    const std::vector<MemOwner::Block> before = m.blocks;
    const int dev0 = f.count(true), pin0 = f.count(false);
    const size_t first = f.sizes.size(), fills0 = f.fills.size();
    f.allocs = f.zeros = 0; f.fail_alloc = atoi(argv[1]); f.fail_fill = atoi(argv[2]);
    const char *err = m.acquire(parts.data(), parts.size());
    f.fail_alloc = f.fail_fill = 0;
    printf("failed %d\n", err != nullptr);
    printf("error %s\n", err ? err : "-");
    printf("pointers_kept %d\n", ptr == prev);
    printf("live_back %d\n", f.count(true) == dev0 && f.count(false) == pin0);
    printf("owner_same %d\n", same(m.blocks, before));
    if (err && retry) {
        // the immediate retry
        f.sizes.resize(first); f.fills.resize(fills0); f.fill_bytes.resize(fills0);
        err = m.acquire(parts.data(), parts.size());
        printf("retry_ok %d\n", err == nullptr);
    }
    if (!err) {
        printf("sizes");
        for (size_t i = first; i < f.sizes.size(); i++) printf(" %zu", f.sizes[i]);
        printf("\nfilled");
        for (size_t k = fills0; k < f.fills.size(); k++)
            for (int i = 0; i < n; i++) if (ptr[i] == f.fills[k]) printf(" %d:%zu", i, f.fill_bytes[k]);
        printf("\n");
        bool owned = m.blocks.size() == before.size() + (size_t)n, distinct = true, pinned_zero = true;
        for (int i = 0; i < n; i++) {
            owned = owned && holds(m, ptr[i]) && f.live.count(ptr[i]) && f.live[ptr[i]].kind == parts[i].kind;
            for (int j = 0; j < i; j++) distinct = distinct && ptr[i] != ptr[j];
            if (parts[i].zero) for (size_t k = 0; k < parts[i].bytes; k++) pinned_zero = pinned_zero && ((unsigned char *)ptr[i])[k] == 0;
        }
        printf("owned %d\ndistinct %d\nzeroed %d\n", owned, distinct, pinned_zero);
        printf("live_grown %d\n", f.count(true) + f.count(false) == dev0 + pin0 + n);
        // one block back: freed once, forgotten, the pointer cleared, nothing else touched
        if (n > 2) {
            const int frees0 = f.frees;
            void *gone = ptr[2];
            m.release(ptr[2]);
            printf("release_one %d\n", f.frees == frees0 + 1 && !f.live.count(gone) && !holds(m, gone) && ptr[2] == nullptr && m.blocks.size() == before.size() + (size_t)n - 1);
            m.release(ptr[2]);                  // (a null pointer: nothing)
            printf("release_null %d\n", f.frees == frees0 + 1);
        }
    }
    // everything back: every block exactly once (the fake aborts on a second free)
    const int live = (int)f.live.size(), frees1 = f.frees;
    m.release_all();
    printf("release_all %d\n", f.frees == frees1 + live && f.live.empty() && m.blocks.empty());
    m.release_all();
    printf("release_all_twice %d\n", f.frees == frees1 + live);
    return 0;
}
'''


def _build(tmp_path_factory, name, extra):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    tmp = tmp_path_factory.mktemp(name)
    src, exe = tmp / 'mem_main.cpp', tmp / 'mem_main'
    src.write_text(DRIVER)
    cmd = ['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-O1', '-g', '-I', CSRC, str(src), '-o', str(exe)] + extra
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0 and extra:
        # the warnings are the plain build's business; here only the sanitizer's runtime may be missing
        probe = tmp / 'probe.cpp'
        probe.write_text('int main() { return 0; }\n')
        if subprocess.run(['g++', str(probe), '-o', str(tmp / 'probe')] + extra, capture_output=True).returncode != 0:
            pytest.skip('g++ %s does not link on this machine' % ' '.join(extra))
    assert done.returncode == 0, done.stderr

    def run(fail_alloc=0, fail_fill=0, retry=1, parts=PARTS):
        args = [str(fail_alloc), str(fail_fill), str(retry)] + [str(x) for part in parts for x in part]
        out = subprocess.run([str(exe)] + args, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        return {line.split(' ', 1)[0]: (line.split(' ', 1) + [''])[1] for line in out.stdout.splitlines()}
    return run


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def owner_program(request, tmp_path_factory):
    """rr_mem.inc compiled ALONE under -Wall -Wextra -Werror, plainly and with the address and undefined-behaviour sanitizers."""
    extra = [] if request.param == 'plain' else ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    return _build(tmp_path_factory, 'mem_' + request.param, extra)


def _check_acquired(r):
    assert r['sizes'].split() == [str(x) for x in REQUESTED]                                  # one allocation per part, bytes + slack
    assert r['filled'].split() == ['%d:%d' % (i, REQUESTED[i]) for i in FILLED]               # fills for exactly the parts that asked
    assert r['owned'] == '1' and r['distinct'] == '1' and r['zeroed'] == '1' and r['live_grown'] == '1'


def test_a_group_is_acquired_whole(owner_program):
    r = owner_program()
    assert r['failed'] == '0'
    _check_acquired(r)
    assert r['release_one'] == '1' and r['release_null'] == '1'
    assert r['release_all'] == '1' and r['release_all_twice'] == '1'


@pytest.mark.parametrize('which,k', [('alloc', k) for k in range(1, N_ALLOCS + 1)] + [('fill', k) for k in range(1, len(FILLED) + 1)])
def test_a_failed_group_changes_nothing_and_the_retry_succeeds(owner_program, which, k):
    r = owner_program(fail_alloc=k if which == 'alloc' else 0, fail_fill=k if which == 'fill' else 0)
    assert r['failed'] == '1' and r['error'].startswith('fake: ')
    assert r['pointers_kept'] == '1'          # every pointer of the list still holds its previous value
    assert r['live_back'] == '1'              # the live count is back where it was
    assert r['owner_same'] == '1'             # the owner is unchanged
    assert r['retry_ok'] == '1'
    _check_acquired(r)
    assert r['release_one'] == '1' and r['release_all'] == '1' and r['release_all_twice'] == '1'


@pytest.mark.parametrize('which,k', [('alloc', 1), ('alloc', N_ALLOCS), ('fill', len(FILLED))])
def test_release_all_after_a_failed_group_is_clean(owner_program, which, k):
    """No retry: the failed group is the last thing the owner saw; release-all then frees the two blocks from before, each once."""
    r = owner_program(fail_alloc=k if which == 'alloc' else 0, fail_fill=k if which == 'fill' else 0, retry=0)
    assert r['failed'] == '1' and 'retry_ok' not in r and 'sizes' not in r
    assert r['live_back'] == '1' and r['owner_same'] == '1'
    assert r['release_all'] == '1' and r['release_all_twice'] == '1'


def test_the_part_has_no_hip_in_it():
    src = open(os.path.join(CSRC, 'rr_mem.inc')).read()
    assert '#include <hip' not in src and 'hipError_t' not in src
    hip = open(os.path.join(CSRC, 'realrobot.hip')).read()
    assert hip.index('#include "rr_mem.inc"') < hip.index('#include "rr_host.inc"')
