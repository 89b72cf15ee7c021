# k_merge_full ordering equal ids by their indices as signed words: of two copies of an id on both sides of 2^31 the
# higher index wins.  tests/test_gpu_extremes.py::test_merge_raised_indices must fail on it (every other test keeps
# its indices below 2^31).
# A test-sensitivity variant for tools/experiments/build_variant.sh: it changes no size, bound or pointer, and no
# test loads it.
s = open("scan.hip").read()
a = '\n                if (!decided && pf[w] != f[w]) { less = pf[w] < f[w]; decided = true; }'
assert s.count(a) == 1
s = s.replace(a, '\n                if (!decided && pf[w] != f[w]) { less = w == DHT_W ? (int)pf[w] < (int)f[w] : pf[w] < f[w]; decided = true; }')
open("scan.hip", "w").write(s)
