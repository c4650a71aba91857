// what the mock of the C ABI saw and what it answers (mock_localmap.cc)
#ifndef MOCK_LOCALMAP_H
#define MOCK_LOCALMAP_H
#include <cstdint>
#include <vector>

#include "orbhip.h"

struct MockLog {
    bool failCreate = false, failSearch = false, hadURight = false;
    int maxPoints = 0, cleared = 0, destroyed = 0, setPuts = 0, searches = 0, setN = 0, setNg = -1;
    uint64_t setKey = 0, frameKey = 0;
    float grid[4] = {0, 0, 0, 0}, nnratio = 0;
    std::vector<orbhip_keypoint> setKps;
    std::vector<uint8_t> setDesc, putDesc, putFlags, flagVals, skip, occupied;
    std::vector<uint64_t> dropped, putKeys, flagKeys, erased, keys;
    std::vector<float> putPos, putNormal, putMin, putMax, uRight;
    orbhip_local_camera cam;
    std::vector<orbhip_local_point> answerPoints;
    std::vector<int32_t> answerMatch;
    int answerToMatch = 0, answerMatches = 0;
};
extern MockLog g_mock;
#endif
