// ofti_draws_layout_check.cpp — the work layout of the OFTI rejection sampler (OftiWork and OftiRows of csrc/draws/octo_draws_layout.h) on host
// memory; tests/test_ofti_draws_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (chunk, N, room) as arguments,
// three numbers a shape (nblk = ⌈N/256⌉, as the driver has it). For each: size the layout with a null base (which must hand out null pointers),
// allocate exactly that many doubles, lay the parts out, fill every element of every part with the part's own tag, read all of them back, and print
// one JSON line with the size, the number of pointers in the struct and each part's offset, element size, length and position in the struct. The
// lengths are stated here, not taken from the header. The rows' layout of N rows follows on a line of its own.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "octo_draws_layout.h"

struct Part {
    const char* name;
    void* p;
    size_t elem;        // bytes of an element
    int64_t len;        // elements
    size_t member;      // offsetof the pointer in its struct
};

#define PART(T, s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(T, m)}

static std::vector<Part> parts_of(const OftiWork& s, int64_t chunk, int64_t N, int64_t nblk, int64_t room) {
    return {PART(OftiWork, s, theta, 5 * chunk), PART(OftiWork, s, nl, 5 * chunk), PART(OftiWork, s, ll, N), PART(OftiWork, s, pmax, nblk),
            PART(OftiWork, s, cnt, nblk + 1), PART(OftiWork, s, max, 1), PART(OftiWork, s, ix, room), PART(OftiWork, s, oll, room), PART(OftiWork, s, olp, room),
            PART(OftiWork, s, otheta, 5 * room), PART(OftiWork, s, onl, 5 * room), PART(OftiWork, s, post, 16 * room)};
}

static void fill(const Part& q, int tag) {
    const int64_t t8 = tag; const int32_t t4 = tag;
    for (int64_t k = 0; k < q.len; ++k) std::memcpy((char*)q.p + k * q.elem, q.elem == 4 ? (const void*)&t4 : (const void*)&t8, q.elem);
}
static bool holds(const Part& q, int tag) {
    const int64_t t8 = tag; const int32_t t4 = tag;
    bool ok = true;
    for (int64_t k = 0; k < q.len; ++k) ok = ok && std::memcmp((const char*)q.p + k * q.elem, q.elem == 4 ? (const void*)&t4 : (const void*)&t8, q.elem) == 0;
    return ok;
}

static void report(const char* layout, const std::vector<Part>& parts, const double* buf, int64_t size, size_t members, const int64_t* shape, int n_shape) {
    std::printf("{\"layout\": \"%s\", \"shape\": [", layout);
    for (int k = 0; k < n_shape; ++k) std::printf("%s%lld", k ? ", " : "", (long long)shape[k]);
    std::printf("], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)size, members);
    for (size_t k = 0; k < parts.size(); ++k) {
        const Part& q = parts[k];
        std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", q.name,
                    (long long)((const char*)q.p - (const char*)buf), q.elem, (long long)q.len, q.member, holds(q, (int)k + 1) ? "true" : "false");
    }
    std::printf("]}\n");
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) return 3;
    for (int a = 1; a + 2 < argc; a += 3) {
        const int64_t chunk = std::atoll(argv[a]), N = std::atoll(argv[a + 1]), room = std::atoll(argv[a + 2]), nblk = (N + 255) / 256;
        {
            const int64_t size = carve_size(ofti_work, chunk, N, nblk, room);
            for (const Part& q : parts_of(carve_at(nullptr, ofti_work, chunk, N, nblk, room), chunk, N, nblk, room)) if (q.p) return 2;
            double* buf = new double[size];
            const OftiWork s = carve_at(buf, ofti_work, chunk, N, nblk, room);
            const std::vector<Part> parts = parts_of(s, chunk, N, nblk, room);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[3] = {chunk, N, room};
            report("ofti_work", parts, buf, size, sizeof(s) / sizeof(void*), shape, 3);
            delete[] buf;
        }
        {
            const int64_t size = carve_size(ofti_rows, N);
            if (carve_at(nullptr, ofti_rows, N).rows) return 2;
            double* buf = new double[size];
            const OftiRows s = carve_at(buf, ofti_rows, N);
            const std::vector<Part> parts = {PART(OftiRows, s, rows, 8 * N)};
            fill(parts[0], 1);
            report("ofti_rows", parts, buf, size, sizeof(s) / sizeof(void*), &N, 1);
            delete[] buf;
        }
    }
    return 0;
}
