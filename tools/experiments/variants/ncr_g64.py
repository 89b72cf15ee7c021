# k_ncr_find: every batch through the wide form (G = 64), for the G crossover of DESIGN.md 5p
s = open("dhtgpu_internal.h").read()
a = "constexpr uint32_t kNcrWideLanes = 64, kNcrNarrowLanes = 16;"
b = [l for l in s.splitlines() if l.startswith("constexpr uint32_t kNcrWideMaxBatch = ")]
assert s.count(a) == 1 and len(b) == 1
s = s.replace(a, "constexpr uint32_t kNcrWideLanes = 64, kNcrNarrowLanes = 16;")
s = s.replace(b[0], "constexpr uint32_t kNcrWideMaxBatch = 0xFFFFFFFFu;")
open("dhtgpu_internal.h", "w").write(s)
