// plan_dump -- prints K6's host planning over a grid of shapes, one line per grid point, through
// the library's own entry points (linked against libdhtgpu; no device is touched).  The prototypes
// are declared here so that the program builds unchanged against any revision of the library:
// tests/test_batch_plan.py compares its output with tests/golden/k6_plan_grid.txt.
//
//   plan_dump            every grid point
//   plan_dump FILE       only the grid points whose key (the text before " |") starts a line of FILE
//
// line: n q_plan k cus nsub pf | supported | rc w0..w15 (nsub == 1, pf == 0; else -) |
//       batch_bytes batch_clean_bytes batch_ctr_offset (supported only; else -) |
//       small_supported small_level small_bytes
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <fstream>
#include <set>
#include <string>

struct dhtgpu_ctx;
extern "C" int dhtgpu_batch_plan(dhtgpu_ctx* ctx, int num_cus, uint64_t n, uint32_t q, uint32_t k, uint32_t out[16]);
namespace dhtgpu {
bool batch_supported(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf);
size_t batch_bytes(uint64_t n, uint32_t q, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf);
size_t batch_clean_bytes(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf);
size_t batch_ctr_offset(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf);
bool small_supported(uint64_t n, uint32_t q, uint32_t k);
uint32_t small_level(uint64_t n, uint32_t k);
size_t small_bytes();
}  // namespace dhtgpu

int main(int argc, char** argv) {
    std::set<std::string> only;
    if (argc > 1) {
        std::ifstream in(argv[1]);
        if (!in) { fprintf(stderr, "plan_dump: cannot read %s\n", argv[1]); return 2; }
        for (std::string line; std::getline(in, line);) {
            const size_t bar = line.find(" |");
            if (bar != std::string::npos) only.insert(line.substr(0, bar));
        }
    }
    const uint64_t ns[] = {1, 5, 40, 1000, 1ull << 15, (1ull << 17) - 1, 1ull << 17, 1ull << 20, (1ull << 24) - 3,
                           1ull << 24, 22400000ull, 1ull << 25, 1ull << 27, (1ull << 31) - 1, 1ull << 31};
    const uint32_t qs[] = {1, 64, 65, 8192, 65536, (1u << 17) - 1, 1u << 17, 1u << 20, 1u << 22, (1u << 22) + 1};
    const uint32_t ks[] = {1, 8, 14, 16, 32, 33};
    const int cus[] = {256, 64, 304, 0};
    const uint32_t nsubs[] = {1, 2, 8, 256, 257};
    for (uint64_t n : ns)
        for (uint32_t qp : qs)
            for (uint32_t k : ks)
                for (int cu : cus)
                    for (uint32_t nsub : nsubs)
                        for (uint32_t pf = 0; pf < 4; ++pf) {
                            char key[128];
                            snprintf(key, sizeof key, "%llu %u %u %d %u %u", (unsigned long long)n, qp, k, cu, nsub, pf);
                            if (argc > 1 && !only.count(key)) continue;
                            const bool sup = dhtgpu::batch_supported(n, qp, k, cu, nsub, pf);
                            printf("%s | %d |", key, sup ? 1 : 0);
                            if (nsub == 1 && pf == 0) {
                                uint32_t w[16] = {0};
                                const int rc = dhtgpu_batch_plan(nullptr, cu, n, qp, k, w);
                                printf(" %d", rc);
                                for (int i = 0; i < 16; ++i) printf(" %u", w[i]);
                            } else {
                                printf(" -");
                            }
                            const uint64_t q = (uint64_t)qp * nsub;
                            if (sup && q <= (1ull << 22))
                                printf(" | %zu %zu %zu", dhtgpu::batch_bytes(n, (uint32_t)q, qp, k, cu, nsub, pf),
                                       dhtgpu::batch_clean_bytes(n, qp, k, cu, nsub, pf),
                                       dhtgpu::batch_ctr_offset(n, qp, k, cu, nsub, pf));
                            else
                                printf(" | -");
                            printf(" | %d %u %zu\n", dhtgpu::small_supported(n, qp, k) ? 1 : 0, dhtgpu::small_level(n, k),
                                   dhtgpu::small_bytes());
                        }
    return 0;
}
