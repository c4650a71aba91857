// The drop-in KeyFrameDatabase called the way LoopClosing::DetectLoop (src/LoopClosing.cc:160-200) and
// Tracking::Relocalization (src/Tracking.cc:2573) call it.  Reads a scenario (argv[1]), one operation per line:
//   add   <id> <n> <word value>...          a new KeyFrame with that mnId and BowVector, then KeyFrameDatabase::add
//   covis <id> <n> <id>...                  its mvpOrderedConnectedKeyFrames (best first)
//   erase <id> | clear
//   reloc <frame id> <n> <word value>...    DetectRelocalizationCandidates(&F)
//   loop  <id> <minScore> <n> <word value>... <m> <connected id>...   DetectLoopCandidates(pKF, minScore) for a query key
//                                           frame that is not in the database
// and writes (argv[2]) per query: "cand <ids...>" and then "kf <id> <mnLoopQuery> <mnLoopWords> <mLoopScore bits>
// <mnRelocQuery> <mnRelocWords> <mRelocScore bits>" for every key frame ever added.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "KeyFrameDatabase.h"
#include "ORBVocabulary.h"
#include "hiperror.h"

using namespace ORB_SLAM2;

static unsigned bits(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

static void read_bow(FILE *in, DBoW2::BowVector &v)
{
    int n = 0;
    if (fscanf(in, "%d", &n) != 1) return;
    for (int i = 0; i < n; i++) {
        unsigned w;
        double x;
        if (fscanf(in, "%u %lf", &w, &x) != 2) return;
        v[w] = x;
    }
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s scenario out vocabulary.bin\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    ORBVocabulary voc;                                         // only size() is read
    if (!voc.loadFromBinaryFile(argv[3])) {
        fprintf(stderr, "vocabulary: %s\n", OrbHipLastError());
        return 3;
    }
    KeyFrameDatabase db(voc);
    std::map<unsigned long, KeyFrame *> kfs;
    char op[16];
    while (fscanf(in, "%15s", op) == 1) {
        std::string o(op);
        if (o == "add") {
            unsigned long id;
            if (fscanf(in, "%lu", &id) != 1) return 4;
            KeyFrame *k = new KeyFrame();
            k->mnId = id;
            read_bow(in, k->mBowVec);
            kfs[id] = k;
            db.add(k);
        } else if (o == "covis") {
            unsigned long id;
            int n;
            if (fscanf(in, "%lu %d", &id, &n) != 2) return 4;
            KeyFrame *k = kfs[id];
            k->mvpOrderedConnectedKeyFrames.clear();
            for (int i = 0; i < n; i++) {
                unsigned long c;
                if (fscanf(in, "%lu", &c) != 1) return 4;
                k->mvpOrderedConnectedKeyFrames.push_back(kfs[c]);
            }
        } else if (o == "erase") {
            unsigned long id;
            if (fscanf(in, "%lu", &id) != 1) return 4;
            db.erase(kfs[id]);
        } else if (o == "clear") {
            db.clear();
        } else if (o == "reloc" || o == "loop") {
            std::vector<KeyFrame *> cand;
            unsigned long id;
            if (fscanf(in, "%lu", &id) != 1) return 4;
            if (o == "reloc") {
                Frame F;
                F.mnId = id;
                read_bow(in, F.mBowVec);
                cand = db.DetectRelocalizationCandidates(&F);   // ref: src/Tracking.cc:2573
            } else {
                float minScore;
                if (fscanf(in, "%f", &minScore) != 1) return 4;
                KeyFrame q;
                q.mnId = id;
                read_bow(in, q.mBowVec);
                int m;
                if (fscanf(in, "%d", &m) != 1) return 4;
                for (int i = 0; i < m; i++) {
                    unsigned long c;
                    if (fscanf(in, "%lu", &c) != 1) return 4;
                    q.mvpOrderedConnectedKeyFrames.push_back(kfs[c]);
                }
                cand = db.DetectLoopCandidates(&q, minScore);    // ref: src/LoopClosing.cc:193
            }
            fprintf(out, "cand");
            for (size_t i = 0; i < cand.size(); i++) fprintf(out, " %lu", cand[i]->mnId);
            fprintf(out, "\n");
            for (std::map<unsigned long, KeyFrame *>::iterator it = kfs.begin(); it != kfs.end(); ++it) {
                KeyFrame *k = it->second;
                fprintf(out, "kf %lu %lu %d %08x %lu %d %08x\n", k->mnId, k->mnLoopQuery, k->mnLoopWords, bits(k->mLoopScore),
                        k->mnRelocQuery, k->mnRelocWords, bits(k->mRelocScore));
            }
        } else {
            return 4;
        }
    }
    fclose(out);
    for (std::map<unsigned long, KeyFrame *>::iterator it = kfs.begin(); it != kfs.end(); ++it) delete it->second;
    return OrbHipErrorCount() ? 5 : 0;
}
