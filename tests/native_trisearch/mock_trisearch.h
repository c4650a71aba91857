// mock_trisearch.h -- what the mock test reads back from the host model of the C entry points (mock_trisearch.cc)
#ifndef ORBHIP_TESTS_MOCK_TRISEARCH_H
#define ORBHIP_TESTS_MOCK_TRISEARCH_H
#include <cstdint>
#include <vector>

#include "orbhip.h"

struct MockLog {
    std::vector<uint64_t> puts;                 // keys of orbhip_set_put, in call order
    std::vector<int> limits;                    // arguments of orbhip_set_limit
    int searches = 0, drops = 0;
    // the last orbhip_search_for_triangulation_sets call
    std::vector<orbhip_tri_neighbour> nb;
    std::vector<uint8_t> skip1, skip2;
    bool ur1Null = true, ur2Null = true;
    std::vector<float> ur2;
};
MockLog &mock_log();
int mock_resident();                            // sets in the model's table
#endif
