// sort_config.h -- the onesweep configuration of the large (u64 key, u32 position) sorts (suffix_sort.hip: round 0;
// record_sort.hip: doubling rounds of 2^23 pairs and more): 9-bit digits, 1024 x 8 items per block; measured 57 ms vs 65 ms
// for rocPRIM's default on 1e9 pairs of 63-bit keys (scripts/micro/sortbench.hip)
#pragma once
#include <rocprim/rocprim.hpp>
using fbg_sort_config = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<512, 32>, rocprim::kernel_config<1024, 8>, 9,
                                        rocprim::block_radix_rank_algorithm::match>>;
