"""CPU: how scripts/kernel_coverage.py spells a kernel's name, and that every kernel which an inventory file under tests/ lists names a test
that exists.  tests/test_libraries_host.py holds each inventory against the library it serves (scripts/kernel_coverage.py checks a profiled
-m gpu run against the same lists); what is left here is what only libmctrain.so has."""
import libraries as L


def test_normalise():
    kc = L.kernel_coverage()
    assert kc.normalise('"void mc::sgm_pass_kernel<0, 4, 0, false, true, 8, true, false>(mc::SgmPassArgs)"') == \
        "sgm_pass_kernel<0, 4, 0, false, true, 8, true, false>"
    assert kc.normalise("void mc::__device_stub__median_kernel<3>(float const*, float*, int, int)") == "median_kernel<3>"
    assert kc.normalise("mc::__device_stub__mean2d_kernel(float const*, float const*, float*, int, int, int, float)") == "mean2d_kernel"
    assert kc.is_library_kernel("void mc::scale_kernel(float const*, float*, long, float)")
    assert not kc.is_library_kernel("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float> >(int)")


def test_every_listed_kernel_names_an_existing_test():
    for name in L.inventory_files():
        inv = L.read_inventory(name)
        assert inv, name
        L.listed_tests_exist(inv)


def test_libmctrains_kernels():
    assert L.built_kernels(L.path("libmctrain.so")) == {"train_sample_kernel", "train_step_kernel<true>", "train_step_kernel<false>", "train_sgd_kernel",
                                                        "gt_filter_kernel", "nnz_count_kernel", "nnz_scan_kernel", "nnz_fill_kernel"}
