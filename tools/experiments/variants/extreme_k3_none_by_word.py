# K3's head() telling an empty slot by its distance words instead of its index: a record at distance {0xFFFFFFFF,
# 0xFFFFFFFF} is dropped.  tests/test_gpu_extremes.py::test_far_lists_merge must fail on it.
# A test-sensitivity variant for tools/experiments/build_variant.sh: it changes no size, bound or pointer, and no
# test loads it.
s = open("scan.hip").read()
a = '        const bool none = ix == DHT_NONE;\n        a = none ? DHT_NONE : my[3 * p] ^ t0;'
assert s.count(a) == 1
s = s.replace(a, '        const bool none = ix == DHT_NONE || ((my[3 * p] ^ t0) == DHT_NONE && (my[3 * p + 1] ^ t1) == DHT_NONE);\n'
                 '        if (none) ix = DHT_NONE;\n        a = none ? DHT_NONE : my[3 * p] ^ t0;')
open("scan.hip", "w").write(s)
