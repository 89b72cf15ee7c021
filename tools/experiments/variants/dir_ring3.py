# k_f2_direct with a ring of 3 sub-steps (48 KB in flight per CU) instead of kF2Ring = 2
s = open("batch.hip").read()
i = s.index("void k_f2_direct(F2Args a)")
j = s.index("// ---- candidate order ----")
body = s[i:j]
assert body.count("kF2Ring") == 5
body = body.replace("kF2Ring", "kDirRingV")
s = s[:i] + body + s[j:]
a = "template <uint32_t Src>\n__global__ __launch_bounds__(kF2Threads) void k_f2_direct(F2Args a)"
assert s.count(a) == 1
s = s.replace(a, "constexpr uint32_t kDirRingV = 3;\n" + a)
open("batch.hip", "w").write(s)
