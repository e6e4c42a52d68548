// dev_buf_test.cpp - host test of dev_buf.h, no GPU and no HIP runtime: the four runtime calls the header makes are
// defined here on top of malloc / free, with a count of live allocations and switches that fail the n-th allocation or
// the next copy.  Built with the host compiler under -fsanitize=address,undefined (make devbuftest); exits 0 when every
// check holds and nothing is left allocated.
#include "../dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

static int g_live = 0;          // allocations not yet freed
static int g_fail_alloc = 0;    // n > 0: the n-th hipMalloc from now fails
static bool g_fail_copy = false;   // the next hipMemcpyAsync fails

extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
    if (g_fail_alloc > 0 && --g_fail_alloc == 0) {
        *p = (void *)0x10;      // what a careless owner would go on to free
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    g_live++;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *p) {
    if (p) {
        g_live--;
        free(p);
    }
    return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
    if (g_fail_copy) {
        g_fail_copy = false;
        return hipErrorInvalidValue;
    }
    memcpy(dst, src, bytes);
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

static int g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            g_bad++;                                                         \
        }                                                                    \
    } while (0)

// a model of the SHT plan: several tables, a container of owners, built member by member with early returns
struct plan {
    dev_buf<double> a, b, c;
    struct cls {
        int len = 0;
        dev_buf<int> list;
    };
    std::vector<cls> classes;
    std::map<int, dev_buf<double>> lazy;
};
static hipError_t plan_build(plan &p, int nclass) {
    hipError_t e;
    if ((e = p.a.alloc(8)) != hipSuccess) return e;
    if ((e = p.b.alloc(8)) != hipSuccess) return e;
    if ((e = p.c.upload(std::vector<double>(5, 1.0), nullptr)) != hipSuccess) return e;
    for (int i = 0; i < nclass; i++) {
        plan::cls c;
        c.len = i;
        if ((e = c.list.upload(std::vector<int>(i, i), nullptr)) != hipSuccess) return e;
        p.classes.push_back(std::move(c));
    }
    return hipSuccess;
}

// a model of ensure_polc: the cache member is both the table and its "built" flag, so it is set last
static hipError_t ensure_table(dev_buf<double> &cache, int *builds) {
    if (cache) return hipSuccess;
    ++*builds;
    const std::vector<double> h(16, 2.0);
    dev_buf<double> t;
    const hipError_t e = t.upload(h, nullptr);
    if (e != hipSuccess) return e;
    cache = std::move(t);
    return hipSuccess;
}

int main() {
    {   // scope exit frees
        dev_buf<double> a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.alloc(4) == hipSuccess && a && g_live == 1);
        double *raw = a;      // the implicit conversion
        CHECK(raw == a.get());
    }
    CHECK(g_live == 0);
    {   // a move leaves exactly one owner
        dev_buf<int> a;
        CHECK(a.alloc(3) == hipSuccess);
        int *raw = a.get();
        dev_buf<int> b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == raw && g_live == 1);
        dev_buf<int> c;
        CHECK(c.alloc(2) == hipSuccess && g_live == 2);
        c = std::move(b);     // frees what c held
        CHECK(b.get() == nullptr && c.get() == raw && g_live == 1);
        dev_buf<int> &self = c;
        c = std::move(self);
        CHECK(c.get() == raw && g_live == 1);
    }
    CHECK(g_live == 0);
    {   // alloc on a held buffer frees the old allocation first; a failed alloc leaves the buffer empty
        dev_buf<double> a;
        CHECK(a.alloc(4) == hipSuccess && a.alloc(8) == hipSuccess && g_live == 1);
        g_fail_alloc = 1;
        CHECK(a.alloc(16) == hipErrorOutOfMemory && !a && g_live == 0);
        CHECK(a.alloc(2) == hipSuccess && g_live == 1);
    }
    CHECK(g_live == 0);
    {   // reset is idempotent
        dev_buf<double> a;
        CHECK(a.reset() == hipSuccess);
        CHECK(a.alloc(1) == hipSuccess);
        CHECK(a.reset() == hipSuccess && !a && g_live == 0);
        CHECK(a.reset() == hipSuccess && g_live == 0);
    }
    {   // upload: max(1, n) elements, the data arrive; a failed copy leaves the buffer empty
        dev_buf<int> a;
        CHECK(a.upload(std::vector<int>(), nullptr) == hipSuccess && a && g_live == 1);
        const std::vector<int> h = {3, 1, 4, 1, 5};
        CHECK(a.upload(h, nullptr) == hipSuccess && g_live == 1 && memcmp(a.get(), h.data(), sizeof(int) * h.size()) == 0);
        g_fail_copy = true;
        CHECK(a.upload(h, nullptr) == hipErrorInvalidValue && !a && g_live == 0);
    }
    CHECK(g_live == 0);
    // a struct of several buffers: a failure in the middle of its construction frees the earlier ones
    for (int fail_at = 1; fail_at <= 6; fail_at++) {
        {
            plan p;
            g_fail_alloc = fail_at;
            CHECK(plan_build(p, 3) == hipErrorOutOfMemory);
            CHECK(g_live == fail_at - 1);
        }
        CHECK(g_live == 0);
    }
    {   // std::vector and std::map of such structs free every element, through reallocation and erase too
        std::map<int, plan> plans;
        for (int k = 0; k < 4; k++) CHECK(plan_build(plans[k], 5) == hipSuccess);
        CHECK(g_live == 4 * (3 + 5));
        CHECK(plans[2].lazy.emplace(7, dev_buf<double>()).first->second.alloc(4) == hipSuccess && g_live == 33);
        plans.erase(1);
        CHECK(g_live == 33 - 8);
        std::vector<plan> v;
        for (int k = 0; k < 9; k++) {
            v.emplace_back();
            CHECK(plan_build(v.back(), 1) == hipSuccess);
        }
        CHECK(g_live == 25 + 9 * 4);
    }
    CHECK(g_live == 0);
    {   // build locally, move in on success: after a failed upload the cache is empty and the next call builds again
        dev_buf<double> cache;
        int builds = 0;
        g_fail_copy = true;
        CHECK(ensure_table(cache, &builds) == hipErrorInvalidValue && !cache && g_live == 0);
        g_fail_alloc = 1;
        CHECK(ensure_table(cache, &builds) == hipErrorOutOfMemory && !cache && g_live == 0);
        CHECK(ensure_table(cache, &builds) == hipSuccess && cache && g_live == 1 && builds == 3);
        CHECK(ensure_table(cache, &builds) == hipSuccess && builds == 3 && cache[15] == 2.0);
    }
    CHECK(g_live == 0);
    if (g_bad || g_live) {
        fprintf(stderr, "dev_buf_test: %d checks failed, %d allocations live at exit\n", g_bad, g_live);
        return 1;
    }
    printf("dev_buf_test OK\n");
    return 0;
}
