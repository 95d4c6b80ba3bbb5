// The owning device buffers of csrc/hpn_ctx.hpp and csrc/hpn_store.hpp (Scratch, InfoBlock, StoreSession, Sorter) over counting,
// malloc-backed stand-ins for the HIP runtime: no HIP library is linked, nothing here touches a device.  Every case ends with no
// live allocation; a pointer freed twice (or by the wrong call) is counted and fails the case.  Prints "ok <case>" per case.
// tests/test_device_buf_host.py builds this with -fsanitize=address,undefined and runs it as a process of its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "hpn_sorter.hpp"

namespace {
std::map<void *, bool> g_live;   // pointer -> pinned host memory?
std::vector<std::string> g_log;  // "malloc" / "free" in the order they came
int g_bad_free = 0, g_fail_malloc = 0, g_fail_memcpy = 0;
size_t g_copied = 0, g_copies = 0;

hipError_t take(void **p, size_t n, bool host)
{
    if (!host && g_fail_malloc) {
        --g_fail_malloc;
        return hipErrorOutOfMemory;
    }
    *p = malloc(n ? n : 1);
    g_live[*p] = host;
    g_log.push_back(host ? "hostmalloc" : "malloc");
    return hipSuccess;
}

hipError_t give(void *p, bool host)
{
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != host) {
        ++g_bad_free;
        return hipErrorInvalidValue;
    }
    g_live.erase(it);
    free(p);
    g_log.push_back(host ? "hostfree" : "free");
    return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return take(p, n, false); }
hipError_t hipFree(void *p) { return give(p, false); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return take(p, n, true); }
hipError_t hipHostFree(void *p) { return give(p, true); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t)
{
    if (g_fail_memcpy) {
        --g_fail_memcpy;
        return hipErrorInvalidValue;
    }
    memcpy(dst, src, n);
    g_copied += n, ++g_copies;
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t)
{
    memset(dst, v, n);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stand-in"; }
}

using namespace hpn;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
            exit(1);                                                    \
        }                                                               \
    } while (0)

namespace {
hpn_ctx g_ctx;
hpn_ctx *const c = &g_ctx;

size_t live() { return g_live.size(); }

template <class T>
T &same(T &x)   // (x = std::move(x) spelt so that no compiler warns about it)
{
    return x;
}

void move_construct()
{
    Scratch a;
    CHECK(scratch_reserve(c, a, 100) == HPN_OK && live() == 1);
    void *p = a.p;
    const size_t cap = a.cap;
    Scratch b(std::move(a));
    CHECK(!a.p && !a.cap && b.p == p && b.cap == cap && live() == 1);
}

void move_assign_live()
{
    Scratch a, b;
    CHECK(scratch_reserve(c, a, 100) == HPN_OK && scratch_reserve(c, b, 200) == HPN_OK && live() == 2);
    void *p = a.p, *old = b.p;
    b = std::move(a);
    CHECK(!a.p && !a.cap && b.p == p && live() == 1 && !g_live.count(old));
}

void self_move()
{
    Scratch a;
    CHECK(scratch_reserve(c, a, 100) == HPN_OK);
    void *p = a.p;
    const size_t cap = a.cap;
    a = std::move(same(a));
    CHECK(a.p == p && a.cap == cap && live() == 1);
    InfoBlock i;
    CHECK(i.alloc(c) == HPN_OK);
    uint32_t *d = i.d;
    i = std::move(same(i));
    CHECK(i.d == d && live() == 3);
}

void release_twice()
{
    Scratch a;
    CHECK(scratch_reserve(c, a, 100) == HPN_OK);
    a.release();
    CHECK(!a.p && !a.cap && live() == 0);
    a.release();
    CHECK(!a.p && !a.cap);
}

void reserve_growth()
{
    Scratch a;
    CHECK(scratch_reserve(c, a, 1000) == HPN_OK && a.cap >= 1000);
    void *p = a.p;
    const size_t n = g_log.size();
    CHECK(scratch_reserve(c, a, a.cap) == HPN_OK && a.p == p && g_log.size() == n);   // within cap: nothing is allocated
    CHECK(scratch_reserve(c, a, a.cap + 1) == HPN_OK && live() == 1);
    CHECK(g_log.size() == n + 2 && g_log[n] == "free" && g_log[n + 1] == "malloc");    // the old buffer goes first
}

void fill(Scratch &s, size_t n)
{
    for (size_t k = 0; k < n; ++k) ((uint8_t *)s.p)[k] = (uint8_t)(k * 7 + 1);
}

bool filled(const Scratch &s, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        if (((const uint8_t *)s.p)[k] != (uint8_t)(k * 7 + 1)) return false;
    return true;
}

void grow_keep_carries()
{
    Scratch a;
    CHECK(grow_keep(c, a, 5000, 0) == HPN_OK && a.cap == ((size_t)1 << 20) && g_copies == 0);
    fill(a, 5000);
    void *old = a.p;
    const size_t n = g_log.size();
    CHECK(grow_keep(c, a, a.cap + 1, 3001) == HPN_OK && a.cap == ((size_t)2 << 20));
    CHECK(g_copies == 1 && g_copied == 3001 && filled(a, 3001) && !g_live.count(old) && live() == 1);
    CHECK(g_log.size() == n + 2 && g_log[n] == "malloc" && g_log[n + 1] == "free");    // (the new one first: the bytes are copied)
    CHECK(grow_keep(c, a, a.cap, 3001) == HPN_OK && g_log.size() == n + 2);
}

void grow_keep_malloc_fails()
{
    Scratch a;
    CHECK(grow_keep(c, a, 5000, 0) == HPN_OK);
    fill(a, 5000);
    void *old = a.p;
    const size_t cap = a.cap;
    g_fail_malloc = 1;
    CHECK(grow_keep(c, a, cap + 1, 5000) == HPN_E_NOMEM && strstr(c->err, "hipMalloc("));
    CHECK(a.p == old && a.cap == cap && filled(a, 5000) && live() == 1 && g_fail_malloc == 0);
}

void grow_keep_copy_fails()
{
    Scratch a;
    CHECK(grow_keep(c, a, 5000, 0) == HPN_OK);
    fill(a, 5000);
    void *old = a.p;
    const size_t cap = a.cap;
    g_fail_memcpy = 1;
    CHECK(grow_keep(c, a, cap + 1, 5000) == HPN_E_HIP);
    CHECK(a.p == old && a.cap == cap && filled(a, 5000) && live() == 1 && g_fail_memcpy == 0);   // the new allocation is gone
}

void info_block()
{
    InfoBlock a;
    CHECK(a.alloc(c) == HPN_OK && live() == 2 && a.ticket() == a.d + kInfoTicket && a.err() == a.d + kInfoErr);
    uint32_t *d = a.d, *h = a.h;
    CHECK(a.alloc(c) == HPN_OK && a.d == d && live() == 2);
    CHECK(a.zero(c) == HPN_OK);
    a.d[kInfoOwn] = 42;
    CHECK(a.fetch(c) == HPN_OK && a.h[kInfoOwn] == 42);
    a.d[kInfoErr] = 1;
    CHECK(a.fetch(c) == HPN_E_HIP && strstr(c->err, "prefix-scan hand-off timed out"));
    CHECK(a.zero(c) == HPN_OK && a.d[kInfoErr] == 0 && a.d[kInfoOwn] == 0);
    InfoBlock b(std::move(a));
    CHECK(!a.d && !a.h && b.d == d && b.h == h && live() == 2);
    InfoBlock e;
    CHECK(e.alloc(c) == HPN_OK && live() == 4);
    e = std::move(b);
    CHECK(!b.d && e.d == d && e.h == h && live() == 2);
}

void grow_stores(StoreSession &s)
{
    for (RecordStore &m : s.m) {
        CHECK(grow_keep(c, m.store, 2 * kStorePad + 100, 0) == HPN_OK && grow_keep(c, m.desc, 64, 0) == HPN_OK);
        m.len = 100, m.pos = 60, m.n = 2, m.closed = true;
    }
    s.open = true;
}

void store_session()
{
    StoreSession s;
    CHECK(s.info.alloc(c) == HPN_OK);
    uint32_t *d = s.info.d;
    grow_stores(s);
    CHECK(live() == 6);
    session_drop(s);
    CHECK(live() == 2 && s.info.d == d && !s.open && !s.finished);
    for (const RecordStore &m : s.m) CHECK(!m.store.p && !m.desc.p && !m.len && !m.pos && !m.n && !m.closed);
    grow_stores(s);
    CHECK(live() == 6);
}

struct Work {   // shaped like a family's: what a new session must not inherit
    Scratch size, out[2];
    uint64_t out_total = 7;
};

struct State : FamilyState, Work {
    StoreSession s;
    Sorter sorter;
};

void drop_session(State *u)   // the family's way
{
    session_drop(u->s);
    static_cast<Work &>(*u) = Work();
    u->sorter.drop();
}

void family_state()
{
    std::unique_ptr<FamilyState> owner(new State);
    State *u = static_cast<State *>(owner.get());
    u->sorter.bytes_only = 1;
    CHECK(u->s.info.alloc(c) == HPN_OK && u->sorter.info.alloc(c) == HPN_OK && u->s.info.d != u->sorter.info.d);
    uint32_t *d = u->s.info.d, *sd = u->sorter.info.d;
    for (int round = 0; round < 2; ++round) {
        grow_stores(u->s);
        CHECK(need(c, u->size, 100) == HPN_OK && need(c, u->out[0], 10) == HPN_OK && need(c, u->out[1], 10) == HPN_OK);
        CHECK(need(c, u->sorter.order, 40) == HPN_OK && need(c, u->sorter.t_kp[1], 80) == HPN_OK);
        u->out_total = 99;
        CHECK(live() == 4 + 4 + 3 + 2);
        drop_session(u);
        CHECK(live() == 4 && u->s.info.d == d && u->sorter.info.d == sd && u->sorter.bytes_only == 1 && u->out_total == 7);
        CHECK(!u->size.p && !u->out[1].p && !u->sorter.order.p && !u->sorter.t_kp[1].p && !u->s.m[1].desc.p);
    }
    grow_stores(u->s);
    CHECK(need(c, u->out[1], 10) == HPN_OK && need(c, u->sorter.key, 80) == HPN_OK && live() == 10);
    owner.reset();   // through the base: everything goes
}

const struct {
    const char *name;
    void (*run)();
} kCases[] = {{"move_construct", move_construct},
              {"move_assign_live", move_assign_live},
              {"self_move", self_move},
              {"release_twice", release_twice},
              {"reserve_growth", reserve_growth},
              {"grow_keep_carries", grow_keep_carries},
              {"grow_keep_malloc_fails", grow_keep_malloc_fails},
              {"grow_keep_copy_fails", grow_keep_copy_fails},
              {"info_block", info_block},
              {"store_session", store_session},
              {"family_state", family_state}};
}  // namespace

int main()
{
    for (const auto &k : kCases) {
        g_log.clear();
        g_copied = g_copies = 0;
        k.run();
        if (live() || g_bad_free) {
            fprintf(stderr, "%s: %zu live allocations, %d bad frees\n", k.name, live(), g_bad_free);
            return 1;
        }
        printf("ok %s\n", k.name);
    }
    return 0;
}
