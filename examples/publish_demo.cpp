// The consumer side of pubKeyframe / pubPointCloud over the C++ mirror (include/vio_adapter.hpp): one camera on the synthetic workload,
// readImage + processLastTracked per frame, then Estimator::keyframe() and Estimator::marginCloud(), each checked bit for bit against one
// vio_publish_all call on the same handle.
// Build:  g++ -std=c++11 -Iinclude examples/publish_demo.cpp -Lvins-rgbd-fast_amd -lvio_hip -Wl,-rpath,$PWD/vins-rgbd-fast_amd
// Usage:  publish_demo [seq] [n_frames]
// Prints one line per processed frame: stamp kf_valid n_kf n_margin n_cloud same   (same = 1: the adapter returned vio_publish_all's bits)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vio_adapter.hpp"
#include "vio_synth.h"

int main(int argc, char **argv) {
    const int seq = argc > 1 ? std::atoi(argv[1]) : 2, n_frames = argc > 2 ? std::atoi(argv[2]) : 30;
    vio_config cfg;
    vio_config_default(&cfg);
    cfg.fix_depth = 0; cfg.depth_max = 10.0;
    vio_synth_config sc;
    vio_synth_config_default(&sc);
    const int nimu = (int)(n_frames / sc.cam_rate * sc.imu_rate) + 64;
    std::vector<double> t(nimu), acc(3 * nimu), gyr(3 * nimu);
    vio_synth_imu(&sc, seq, nimu, t.data(), acc.data(), gyr.data());
    std::vector<uint8_t> gray((size_t)cfg.width * cfg.height);
    std::vector<uint16_t> depth((size_t)cfg.width * cfg.height);
    try {
        vio_hip::Estimator estimator(cfg);
        vio_hip::FeatureTracker tracker(estimator);
        estimator.setParameter();
        int32_t capacity[3];
        if (vio_get_capacity(estimator.handle(), capacity) != VIO_OK) return 1;
        const int cap = capacity[1];
        std::vector<double> cloud(3 * (size_t)cap), margin(3 * (size_t)cap), points(8 * (size_t)cap);
        int k = 0;
        for (int fm = 1; fm < n_frames; fm++) {
            const double stamp = fm / sc.cam_rate;
            while (k < nimu && t[k] < stamp + 1.5 / sc.imu_rate) { estimator.inputIMU(t[k], &acc[3 * k], &gyr[3 * k]); k++; }
            vio_synth_render_host(&sc, seq, stamp, gray.data(), depth.data());
            tracker.readImage(gray.data(), stamp);
            if (fm < 3) continue;   // the nodelet drops the first two published maps (estimator_nodelet.cpp:365-377)
            if (estimator.processLastTracked(depth.data()) == VIO_NEED_IMU) continue;
            const vio_hip::Estimator::Keyframe kf = estimator.keyframe();
            const std::vector<double> mc = estimator.marginCloud(), pc = estimator.pointCloud();
            int32_t counts[4];
            double pose[8];
            std::memset(pose, 0, sizeof(pose));
            if (vio_publish_all(estimator.handle(), cap, counts, pose, cloud.data(), margin.data(), points.data(), 0) != VIO_OK) return 1;
            bool same = kf.valid == (counts[3] != 0) && kf.points.size() == 8 * (size_t)counts[2] && mc.size() == 3 * (size_t)counts[1] &&
                        pc.size() == 3 * (size_t)counts[0];
            same = same && std::memcmp(kf.pose, pose, sizeof(pose)) == 0;
            same = same && (kf.points.empty() || std::memcmp(kf.points.data(), points.data(), kf.points.size() * sizeof(double)) == 0);
            same = same && (mc.empty() || std::memcmp(mc.data(), margin.data(), mc.size() * sizeof(double)) == 0);
            std::printf("%.4f %d %d %d %d %d\n", stamp, (int)counts[3], (int)counts[2], (int)counts[1], (int)counts[0], same ? 1 : 0);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
