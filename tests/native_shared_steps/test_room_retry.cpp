// test_room_retry -- room_for and call_with_room of host/localmap/LocalMapDetail.h on their own: how much room a call of the
// LocalMapSearch drop-ins offers first, and when the call is made again.  Links nothing of the class; the
// "entry point" is a callable that reports a list of a given length and answers as the C ABI does.  Prints "ok".
#include <cstdio>
#include <vector>

#include "LocalMapDetail.h"

using ORB_SLAM2::localmapdetail::call_with_room;
using ORB_SLAM2::localmapdetail::room_for;

namespace
{
int g_failed = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            g_failed++;                                               \
        }                                                             \
    } while (0)

// what an entry point with a capacity argument does: reports the list's length, fills no more than the room it was given (so
// that the sanitizer twin sees a buffer smaller than promised), answers ORBHIP_E_CAPACITY when the list does not fit
struct Entry {
    std::vector<int> lengths;   // the list's length at the first, second, ... call (the last one repeats)
    int error;                  // returned instead of ORBHIP_OK / ORBHIP_E_CAPACITY from call `errorAt` on
    size_t errorAt;
    std::vector<int> caps;      // the capacities seen, in order
    std::vector<size_t> rooms;  // the buffer sizes seen, in order
    std::vector<int> buf;
    int reported;
    Entry() : error(ORBHIP_OK), errorAt((size_t)-1), reported(0) {}
    int operator()(int cap, size_t room)
    {
        const size_t call = caps.size();
        caps.push_back(cap), rooms.push_back(room);
        buf.assign(room, -1);
        buf.shrink_to_fit();
        const int n = lengths[call < lengths.size() ? call : lengths.size() - 1];
        reported = n;
        if (call >= errorAt) return error;
        for (int i = 0; i < n && i < cap; i++) buf[i] = i;
        return n > cap ? ORBHIP_E_CAPACITY : ORBHIP_OK;
    }
};

int run(Entry &e, int cap)
{
    return call_with_room(cap, &e.reported, [&](int c, size_t room) { return e(c, room); });
}

std::vector<int> ints(int a) { return std::vector<int>(1, a); }
std::vector<int> ints(int a, int b) { std::vector<int> v(1, a); v.push_back(b); return v; }
std::vector<int> ints(int a, int b, int c) { std::vector<int> v = ints(a, b); v.push_back(c); return v; }
}  // namespace

int main()
{
    // ---- room_for: a quarter more than last time and the slack, never more than there is ----
    CHECK(room_for(0, 100000) == 256);
    CHECK(room_for(4, 100000) == 4 + 1 + 256);
    CHECK(room_for(3, 100000) == 3 + 0 + 256);
    CHECK(room_for(1000, 100000) == 1000 + 250 + 256);
    CHECK(room_for(1000, 700) == 700);            // most < last
    CHECK(room_for(1000, 1300) == 1300);          // most between last and last's room
    CHECK(room_for(1000, 0) == 0);                // most == 0
    CHECK(room_for(0, 0) == 0);
    CHECK(room_for(0, 100000, 16) == 16);         // UpdateConnections' slack, per query
    CHECK(room_for(40, 100000, 16) == 40 + 10 + 16);
    CHECK(room_for(40, 50, 16) == 50);
    CHECK(7 * room_for(40, 100000, 16) == 7 * 66);   // ... and its factor stays at the site

    // ---- call_with_room ----
    {   // enough room at once: one call
        Entry e;
        e.lengths = ints(200);
        CHECK(run(e, 256) == ORBHIP_OK);
        CHECK(e.caps == ints(256) && e.rooms == std::vector<size_t>(1, 256) && e.reported == 200);
    }
    {   // exactly enough is enough
        Entry e;
        e.lengths = ints(256);
        CHECK(run(e, 256) == ORBHIP_OK && e.caps == ints(256));
    }
    {   // too little once: the second call has exactly the reported count
        Entry e;
        e.lengths = ints(1000);
        CHECK(run(e, 256) == ORBHIP_OK);
        CHECK(e.caps == ints(256, 1000) && e.rooms.back() == 1000 && e.reported == 1000);
    }
    {   // too little twice in a row (the list grew between the calls): three calls
        Entry e;
        e.lengths = ints(1000, 1500);
        CHECK(run(e, 256) == ORBHIP_OK);
        CHECK(e.caps == ints(256, 1000, 1500) && e.rooms.back() == 1500 && e.reported == 1500);
    }
    {   // ORBHIP_E_CAPACITY with a count that is not above the capacity: returned, no second call
        Entry e;
        e.lengths = ints(100);
        e.error = ORBHIP_E_CAPACITY, e.errorAt = 0;
        CHECK(run(e, 256) == ORBHIP_E_CAPACITY && e.caps == ints(256));
        Entry same;
        same.lengths = ints(256);
        same.error = ORBHIP_E_CAPACITY, same.errorAt = 0;
        CHECK(run(same, 256) == ORBHIP_E_CAPACITY && same.caps == ints(256));
    }
    {   // another error: returned, one call, whatever the count says
        Entry e;
        e.lengths = ints(1000);
        e.error = ORBHIP_E_HIP, e.errorAt = 0;
        CHECK(run(e, 256) == ORBHIP_E_HIP && e.caps == ints(256));
    }
    {   // another error at the second call: returned, two calls
        Entry e;
        e.lengths = ints(1000);
        e.error = ORBHIP_E_ARG, e.errorAt = 1;
        CHECK(run(e, 256) == ORBHIP_E_ARG && e.caps == ints(256, 1000));
    }
    {   // capacity 0: the callable is told 0 and still gets a buffer of one element
        Entry e;
        e.lengths = ints(0);
        CHECK(run(e, 0) == ORBHIP_OK);
        CHECK(e.caps == ints(0) && e.rooms == std::vector<size_t>(1, 1));
        Entry grow;
        grow.lengths = ints(3);
        CHECK(run(grow, 0) == ORBHIP_OK);
        CHECK(grow.caps == ints(0, 3) && grow.rooms[0] == 1 && grow.rooms[1] == 3);
    }
    if (g_failed) return 1;
    printf("ok\n");
    return 0;
}
