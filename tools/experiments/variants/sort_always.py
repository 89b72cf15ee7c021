# sub-partitions always built prefix-sorted (the sort decision's threshold, whatever it is, -> 0):
# the prefix / shard shapes then take k_f2_direct too
import re
s = open("api.hip").read()
a = re.compile(r"(sort = 1\.0 - std::exp\(-qsub / \(double\)\(1ull << lm\)\) > )[0-9.]+;")
assert len(a.findall(s)) == 1
s = a.sub(r"\g<1>0.0;", s)
open("api.hip", "w").write(s)
