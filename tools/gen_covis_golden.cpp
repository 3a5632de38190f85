// Writes tests/golden/covis_ref.npz: about 100 small maps built with the REFERENCE's own KeyFrame, MapPoint and Map objects,
// recorded as our tables, with what the compiled reference answers on them:
//   Map::compareViewMPs(pKF1, pKF2, spMPs)            for every ordered pair of key frames of every map
//   Map::compareViewMPs(pKF, spKFsRef, spMPsRet, 2)   for every key frame against a recorded reference set
//   Map::updateCovisibility(pNewKF)                   the covisible key frames it adds for the last key frame of every map
//                                                     against a recorded mLocalGraphKFs
// The program includes the reference's headers where they lie ($REF = the reference's checkout) and links
// oracle/_ref/libse2lam_ref_map.so (built by the oracle recipe: the reference's Map.cpp, KeyFrame.cpp, MapPoint.cpp); nothing
// of the reference is copied here.  Built by hand, from the repository's root:
//   g++ -std=c++14 -O2 -ffp-contract=off -w -I oracle/_shim -I $REF/include/se2lam -I $REF -include oracle/_shim/se2lam_stubs_map.h \
//       tools/gen_covis_golden.cpp oracle/_ref/libse2lam_ref_map.so -Wl,-rpath,$PWD/oracle/_ref -lpthread \
//       -o build/gen_covis_golden && build/gen_covis_golden tests/golden/covis_ref.npz
// Only the key frame's side is filled (KeyFrame::addObservation): compareViewMPs reads nothing else.  A null point is one
// whose MapPoint::setNull(pThis) ran while its own observation list was empty, so the key frames keep their entries - the state
// a point is in between MapPoint::setNull and the next sweep of the map.
// Arrays (i4 unless said; obs_frame, obs_ftr, pair_common and job_common u1; "off" arrays index the array named after them and
// have one more entry than items):
//   cap (1), kf_off (nmaps + 1) -> counts;  mp_off -> mp_null / good_prl (u1);  ptr_off -> mp_ptr (m + 1 per map, relative
//   to the map's first observation);  obs_off -> obs_frame / obs_ftr
//   CSR order: point by point, within a point key frame by key frame, each key frame's getObservations() being the source
//   pair_off (nmaps + 1) -> the nkf * nkf ordered pairs (a major) of a map: pair_ratio (N, 2) f4, pair_common_off -> pair_common
//   job_off = kf_off: per key frame ref_off -> ref_idx, job_ratio f8, job_common_off -> job_common
//   new_kf (nmaps), local_off -> local_kfs, connect_off -> connect (ascending slots)
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"

using namespace se2lam;

// ---- a .npz is a zip archive of .npy files; stored without compression
static uint32_t crc32_of(const std::string& s) {
    uint32_t c = 0xffffffffu;
    for (unsigned char ch : s) {
        c ^= ch;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}
static void put(std::string& o, uint32_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) o.push_back((char)((v >> (8 * k)) & 0xff));
}
struct Npz {
    std::string body, central;
    int count = 0;
    void add(const std::string& name, const char* descr, size_t rows, size_t cols, const void* data, size_t bytes) {
        std::string shape = cols ? "(" + std::to_string(rows) + ", " + std::to_string(cols) + ")" : "(" + std::to_string(rows) + ",)";
        std::string h = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
        while ((10 + h.size() + 1) % 64) h.push_back(' ');
        h.push_back('\n');
        std::string f("\x93NUMPY\x01\x00", 8);
        put(f, (uint32_t)h.size(), 2);
        f += h;
        f.append((const char*)data, bytes);
        const std::string fn = name + ".npy";
        const uint32_t crc = crc32_of(f), off = (uint32_t)body.size();
        put(body, 0x04034b50u, 4); put(body, 20, 2); put(body, 0, 2); put(body, 0, 2); put(body, 0, 2); put(body, 0x21, 2);
        put(body, crc, 4); put(body, (uint32_t)f.size(), 4); put(body, (uint32_t)f.size(), 4); put(body, (uint32_t)fn.size(), 2);
        put(body, 0, 2);
        body += fn;
        body += f;
        put(central, 0x02014b50u, 4); put(central, 20, 2); put(central, 20, 2); put(central, 0, 2); put(central, 0, 2);
        put(central, 0, 2); put(central, 0x21, 2); put(central, crc, 4); put(central, (uint32_t)f.size(), 4);
        put(central, (uint32_t)f.size(), 4); put(central, (uint32_t)fn.size(), 2); put(central, 0, 2); put(central, 0, 2);
        put(central, 0, 2); put(central, 0, 2); put(central, 0, 4); put(central, off, 4);
        central += fn;
        ++count;
    }
    void ints(const std::string& name, const std::vector<int32_t>& v) { add(name, "<i4", v.size(), 0, v.data(), 4 * v.size()); }
    void bytes(const std::string& name, const std::vector<uint8_t>& v) { add(name, "|u1", v.size(), 0, v.data(), v.size()); }
    bool write(const char* path) {
        std::string end;
        put(end, 0x06054b50u, 4); put(end, 0, 2); put(end, 0, 2); put(end, (uint32_t)count, 2); put(end, (uint32_t)count, 2);
        put(end, (uint32_t)central.size(), 4); put(end, (uint32_t)body.size(), 4); put(end, 0, 2);
        FILE* f = std::fopen(path, "wb");
        if (!f) return false;
        const std::string all = body + central + end;
        const bool ok = std::fwrite(all.data(), 1, all.size(), f) == all.size();
        return std::fclose(f) == 0 && ok;
    }
};

struct MapAccess : public Map {          // mLocalGraphKFs is protected: what Map::updateLocalGraph would have left there
    void setLocal(const std::vector<PtrKeyFrame>& v) { mLocalGraphKFs = v; }
};

static const int CAP = 64;

static PtrKeyFrame make_kf() {
    Frame f;
    f.N = CAP;
    f.keyPoints.resize(CAP);
    f.keyPointsUn = f.keyPoints;
    f.descriptors = cv::Mat::zeros(CAP, 32, CV_8UC1);
    f.Tcw = cv::Mat::eye(4, 4, CV_32FC1);
    f.Tcr = cv::Mat::eye(4, 4, CV_32FC1);
    return std::make_shared<KeyFrame>(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::mt19937 rng(20240607u);
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };   // inclusive
    auto coin = [&](double p) { return (rng() >> 8) * (1.0 / 16777216.0) < p; };
    std::vector<int32_t> cap{CAP}, kf_off{0}, counts, mp_off{0}, ptr_off{0}, mp_ptr, obs_off{0};
    std::vector<uint8_t> mp_null, good_prl, obs_frame, obs_ftr, pair_common, job_common;   // slots < 8, features < 64, points < 60
    std::vector<int32_t> pair_off{0}, pair_common_off{0}, ref_off{0}, ref_idx, job_common_off{0};
    std::vector<float> pair_ratio;
    std::vector<double> job_ratio;
    std::vector<int32_t> new_kf, local_off{0}, local_kfs, connect_off{0}, connect;
    const int NMAPS = 100;
    for (int im = 0; im < NMAPS; ++im) {
        const int nkf = im % 10 == 9 ? 8 : uni(2, 5), nmp = im == 0 ? 0 : im == 1 ? 1 : im % 10 == 8 ? 60 : uni(3, 36);
        const double pobs = 0.15 + 0.8 * ((im * 7) % 10) / 9.0;
        std::vector<PtrKeyFrame> kfs;
        std::vector<PtrMapPoint> mps;
        for (int f = 0; f < nkf; ++f) kfs.push_back(make_kf());
        std::vector<uint8_t> isnull(nmp, 0);
        for (int p = 0; p < nmp; ++p) {
            mps.push_back(std::make_shared<MapPoint>(cv::Point3f(0.f, 0.f, 3.f), !coin(0.25)));
            isnull[p] = coin(0.12);
        }
        std::vector<int> nxt(nkf, 0);
        for (int f = 0; f < nkf; ++f)
            for (int p = 0; p < nmp; ++p)
                if (nxt[f] < CAP && coin(pobs)) kfs[f]->addObservation(mps[p], nxt[f]++);
        for (int p = 0; p < nmp; ++p)
            if (isnull[p]) mps[p]->setNull(mps[p]);
        // ---- our tables, from the key frames' own containers
        std::map<PtrMapPoint, int> index;
        for (int p = 0; p < nmp; ++p) index[mps[p]] = p;
        std::vector<std::vector<std::pair<int, int>>> lists(nmp);
        for (int f = 0; f < nkf; ++f) {
            const std::map<PtrMapPoint, int> obs = kfs[f]->getObservations();
            for (const auto& o : obs) lists[index.at(o.first)].push_back(std::make_pair(f, o.second));
            counts.push_back(CAP);
        }
        int nobs = 0;
        mp_ptr.push_back(0);
        for (int p = 0; p < nmp; ++p) {
            for (const auto& e : lists[p]) {
                obs_frame.push_back((uint8_t)e.first);
                obs_ftr.push_back((uint8_t)e.second);
            }
            nobs += (int)lists[p].size();
            mp_ptr.push_back(nobs);
            mp_null.push_back(mps[p]->isNull() ? 1 : 0);
            good_prl.push_back(mps[p]->isGoodPrl() ? 1 : 0);
        }
        kf_off.push_back((int32_t)counts.size());
        mp_off.push_back((int32_t)mp_null.size());
        ptr_off.push_back((int32_t)mp_ptr.size());
        obs_off.push_back((int32_t)obs_frame.size());
        // ---- the reference's answers
        for (int a = 0; a < nkf; ++a)
            for (int b = 0; b < nkf; ++b) {
                std::set<PtrMapPoint> sp;
                const cv::Point2f r = Map::compareViewMPs(kfs[a], kfs[b], sp);
                pair_ratio.push_back(r.x);
                pair_ratio.push_back(r.y);
                std::set<int> pts;
                for (const auto& q : sp) pts.insert(index.at(q));
                pair_common.insert(pair_common.end(), pts.begin(), pts.end());
                pair_common_off.push_back((int32_t)pair_common.size());
            }
        pair_off.push_back((int32_t)pair_common_off.size() - 1);
        for (int f = 0; f < nkf; ++f) {
            std::set<PtrKeyFrame> refs;
            const double pref = im % 3 == 0 ? 0.9 : 0.5;
            for (int g = 0; g < nkf; ++g)
                if ((g != f || coin(0.2)) && coin(pref)) {
                    refs.insert(kfs[g]);
                    ref_idx.push_back(g);
                }
            ref_off.push_back((int32_t)ref_idx.size());
            std::set<PtrMapPoint> sp;
            job_ratio.push_back(Map::compareViewMPs(kfs[f], refs, sp, 2));
            std::set<int> pts;
            for (const auto& q : sp) pts.insert(index.at(q));
            job_common.insert(job_common.end(), pts.begin(), pts.end());
            job_common_off.push_back((int32_t)job_common.size());
        }
        MapAccess map;
        std::vector<PtrKeyFrame> local;
        for (int g = 0; g + 1 < nkf; ++g)
            if (coin(0.8)) {
                local.push_back(kfs[g]);
                local_kfs.push_back(g);
            }
        local_off.push_back((int32_t)local_kfs.size());
        map.setLocal(local);
        new_kf.push_back(nkf - 1);
        map.updateCovisibility(kfs[nkf - 1]);
        const std::set<PtrKeyFrame> cov = kfs[nkf - 1]->getAllCovisibleKFs();
        for (int g = 0; g < nkf; ++g)
            if (cov.count(kfs[g])) {
                connect.push_back(g);
                if (!kfs[g]->getAllCovisibleKFs().count(kfs[nkf - 1])) return 3;   // :795-796 connect both ways
            }
        connect_off.push_back((int32_t)connect.size());
    }
    Npz z;
    z.ints("cap", cap); z.ints("kf_off", kf_off); z.ints("counts", counts); z.ints("mp_off", mp_off);
    z.bytes("mp_null", mp_null); z.bytes("good_prl", good_prl); z.ints("ptr_off", ptr_off); z.ints("mp_ptr", mp_ptr);
    z.ints("obs_off", obs_off); z.bytes("obs_frame", obs_frame); z.bytes("obs_ftr", obs_ftr);
    z.ints("pair_off", pair_off); z.add("pair_ratio", "<f4", pair_ratio.size() / 2, 2, pair_ratio.data(), 4 * pair_ratio.size());
    z.ints("pair_common_off", pair_common_off); z.bytes("pair_common", pair_common);
    z.ints("ref_off", ref_off); z.ints("ref_idx", ref_idx);
    z.add("job_ratio", "<f8", job_ratio.size(), 0, job_ratio.data(), 8 * job_ratio.size());
    z.ints("job_common_off", job_common_off); z.bytes("job_common", job_common);
    z.ints("new_kf", new_kf); z.ints("local_off", local_off); z.ints("local_kfs", local_kfs);
    z.ints("connect_off", connect_off); z.ints("connect", connect);
    if (!z.write(argv[1])) return 1;
    std::printf("%s: %d maps, %zu key frames, %zu points, %zu observations, %zu pairs\n", argv[1], NMAPS, counts.size(),
                mp_null.size(), obs_frame.size(), pair_ratio.size() / 2);
    return 0;
}
