// Writes tests/golden/view_info_ref.npz: about 200 inputs of Track::calcSE3toXYZInfo with the two informations the
// REFERENCE computes for them.  The program links oracle/_ref/libse2lam_ref_map.so (built by the oracle recipe, it holds the
// reference's Track.cpp) and calls the static se2lam::Track::calcSE3toXYZInfo and cvu::inv; the class is declared here with
// that one member, which gives the same symbol.  The cv::Mat arithmetic behind the numbers is the stand-in's
// (oracle/_shim/cv_shim.cpp), not OpenCV's.
//   g++ -std=c++14 -O2 -ffp-contract=off -I oracle/_shim tools/gen_view_info_golden.cpp oracle/_ref/libse2lam_ref_map.so \
//       -Wl,-rpath,$PWD/oracle/_ref -o build/gen_view_info_golden && build/gen_view_info_golden tests/golden/view_info_ref.npz
// Arrays: xyz1 (n, 3) f4, Tcw1 / Tcw2 / Twc1 / Twc2 (n, 12) f4 (rows 0-2; Twc = cvu::inv(Tcw)), fx (n) f4,
//         info1 / info2 (n, 9) f8 row-major, depth / off_axis_deg / baseline (n) f4 describing the case.
#include <Eigen/Core>
#include <opencv2/core/core.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace se2lam {
class Track {
public:
    static void calcSE3toXYZInfo(cv::Point3f xyz1, const cv::Mat& Tcw1, const cv::Mat& Tcw2, Eigen::Matrix3d& info1,
                                 Eigen::Matrix3d& info2);
};
struct Config {
    static float fxCam;
};
}  // namespace se2lam
namespace cvu {
cv::Mat inv(const cv::Mat& T4x4);
}

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

static cv::Mat pose(double yaw, double pitch, double cx, double cy, double cz) {
    const double cyw = std::cos(yaw), syw = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
    const double Ry[9] = {cyw, 0, syw, 0, 1, 0, -syw, 0, cyw}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = Rx[3 * r] * Ry[c] + Rx[3 * r + 1] * Ry[3 + c] + Rx[3 * r + 2] * Ry[6 + c];
    const double C[3] = {cx, cy, cz};
    cv::Mat T = cv::Mat::eye(4, 4, CV_32FC1);
    for (int r = 0; r < 3; ++r) {
        double t = 0;
        for (int c = 0; c < 3; ++c) {
            T.at<float>(r, c) = (float)R[3 * r + c];
            t -= R[3 * r + c] * C[c];
        }
        T.at<float>(r, 3) = (float)t;
    }
    return T;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const float depths[5] = {0.8f, 2.f, 5.f, 12.f, 30.f};
    const float angles[5] = {0.5f, 5.f, 12.f, 22.f, 35.f};          // degrees off the optical axis of camera 1
    const float baselines[4] = {0.05f, 0.2f, 0.6f, 1.5f};
    std::mt19937 rng(20240607);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<float> xyz1, T1, T2, W1, W2, fx, dep, ang, bas;
    std::vector<double> I1, I2;
    for (int di = 0; di < 5; ++di)
        for (int ai = 0; ai < 5; ++ai)
            for (int bi = 0; bi < 4; ++bi)
                for (int rep = 0; rep < 2; ++rep) {
                    const double a = angles[ai] * M_PI / 180.0, dir = M_PI * u(rng), d = depths[di];
                    const cv::Point3f p((float)(d * std::tan(a) * std::cos(dir)), (float)(d * std::tan(a) * std::sin(dir)), (float)d);
                    const cv::Mat Tcw1 = rep ? pose(0.3 * u(rng), 0.1 * u(rng), u(rng), 0.2 * u(rng), u(rng)) : cv::Mat(cv::Mat::eye(4, 4, CV_32FC1));
                    // camera 2: camera 1 moved by the baseline across its optical axis (plus a little along it) and turned
                    const cv::Mat Twc1 = cvu::inv(Tcw1);
                    const double bx = baselines[bi] * std::cos(dir + 0.7), by = 0.3 * baselines[bi] * std::sin(dir + 0.7), bz = 0.2 * baselines[bi] * u(rng);
                    const cv::Mat T21 = pose(0.1 * u(rng), 0.03 * u(rng), bx, by, bz);   // camera 2 in camera 1's frame
                    const cv::Mat Tcw2 = cv::Mat(T21 * Tcw1);
                    const cv::Mat Twc2 = cvu::inv(Tcw2);
                    const float f = rep ? 230.f + 200.f * (float)std::fabs(u(rng)) : 230.f;
                    se2lam::Config::fxCam = f;
                    Eigen::Matrix3d i1, i2;
                    se2lam::Track::calcSE3toXYZInfo(p, Tcw1, Tcw2, i1, i2);
                    xyz1.insert(xyz1.end(), {p.x, p.y, p.z});
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 4; ++c) {
                            T1.push_back(Tcw1.at<float>(r, c)); T2.push_back(Tcw2.at<float>(r, c));
                            W1.push_back(Twc1.at<float>(r, c)); W2.push_back(Twc2.at<float>(r, c));
                        }
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 3; ++c) { I1.push_back(i1(r, c)); I2.push_back(i2(r, c)); }
                    fx.push_back(f); dep.push_back(depths[di]); ang.push_back(angles[ai]); bas.push_back(baselines[bi]);
                }
    const size_t n = fx.size();
    Npz z;
    z.add("xyz1", "<f4", n, 3, xyz1.data(), xyz1.size() * 4);
    z.add("Tcw1", "<f4", n, 12, T1.data(), T1.size() * 4);
    z.add("Tcw2", "<f4", n, 12, T2.data(), T2.size() * 4);
    z.add("Twc1", "<f4", n, 12, W1.data(), W1.size() * 4);
    z.add("Twc2", "<f4", n, 12, W2.data(), W2.size() * 4);
    z.add("fx", "<f4", n, 0, fx.data(), fx.size() * 4);
    z.add("info1", "<f8", n, 9, I1.data(), I1.size() * 8);
    z.add("info2", "<f8", n, 9, I2.data(), I2.size() * 8);
    z.add("depth", "<f4", n, 0, dep.data(), dep.size() * 4);
    z.add("off_axis_deg", "<f4", n, 0, ang.data(), ang.size() * 4);
    z.add("baseline", "<f4", n, 0, bas.data(), bas.size() * 4);
    if (!z.write(argv[1])) return 1;
    std::printf("%zu cases -> %s\n", n, argv[1]);
    return 0;
}
