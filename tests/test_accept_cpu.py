"""CPU-side check of the accept mask: the C++11 adapter's accept-mask members
(tests/cpp/accept_check.cpp, built against a mock node type; no device is touched).  The entry
points' declaration, export and binding: tests/test_abi.py; the view kernels' register and scratch
budget: tests/test_kernel_resources.py."""
import subprocess

import cpp_check


def test_cpp_accept_adapter_compiles(tmp_path):
    """ClosestIndex::set_accept / clear_accept / update_accept / write / set_accept_good compile as
    C++11 with -Wall -Wextra -Werror against a mock node type that has isGood(now)."""
    exe = cpp_check.build("accept", tmp_path)
    assert subprocess.check_output([exe], text=True).strip() == "built"
