// Host build of csrc/relink_config.h, the argument checks and the config copy of mpe_relink_create, for a run under
// -fsanitize=address,undefined (tests/test_relink_host.py).  Every bone list sits in a heap buffer of exactly its size, so a
// read past n_bones pairs is a report.  Prints "ok <checks>" and exits 0, or says what differed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "relink_config.h"

namespace {

int checks = 0, failures = 0;

void expect(const mpe_relink_config &c, int code, const char *word, const char *what) {
    char why[400] = "";
    const int rc = mpe::relink_check_config(&c, why, sizeof why);
    ++checks;
    if (rc != code || (word && !strstr(why, word))) {
        printf("%s: code %d (want %d), message '%s' (want '%s')\n", what, rc, code, why, word ? word : "");
        ++failures;
    }
}

}  // namespace

int main() {
    const int n = 18;
    std::unique_ptr<int32_t[]> bones(new int32_t[2 * n]);
    for (int b = 0; b < n; ++b) {
        bones[2 * b] = b == 0 ? 17 : b - 1;
        bones[2 * b + 1] = b == 0 ? 0 : b;
    }
    mpe_relink_config good{};
    good.pcap = 10; good.n_joints = 18; good.pose_f64 = 1; good.tid_cap = 256; good.n_bones = n; good.max_frames = 1024;
    good.min_gap = 4; good.max_gap = 150; good.min_samples = 5; good.min_bones = 8;
    good.used_joint_mask = 0x3FFE1u; good.joint_mask = 0xFFFFFFFFu;
    good.gate_m = 0.02; good.max_bone_m = 1.0; good.reach_m = 0.0; good.reach_per_frame_m = 0.0;
    good.bones = bones.get();
    expect(good, MPE_OK, nullptr, "defaults");
    char why[8];
    ++checks;
    if (mpe::relink_check_config(nullptr, why, sizeof why) != MPE_ERR_INVALID || strcmp(why, "NULL ar") != 0) {     // cut to the buffer
        printf("NULL config: '%s'\n", why);
        ++failures;
    }
    mpe_relink_config c = good;
    c.bones = nullptr;
    expect(c, MPE_ERR_INVALID, "NULL", "NULL bones");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
#define BAD(field, value, code, word)      \
    c = good;                              \
    c.field = value;                       \
    expect(c, code, word, #field " = " #value)
    BAD(pcap, 0, MPE_ERR_INVALID, "pcap 0");
    BAD(pcap, 129, MPE_ERR_CAPACITY, "pcap 129");
    BAD(n_joints, 33, MPE_ERR_INVALID, "joints 33");
    BAD(pose_f64, 2, MPE_ERR_INVALID, "pose_f64 2");
    BAD(tid_cap, 0, MPE_ERR_INVALID, "tid_cap 0");
    BAD(tid_cap, 4097, MPE_ERR_CAPACITY, "tid_cap 4097");
    BAD(n_bones, 0, MPE_ERR_INVALID, "n_bones 0");
    BAD(n_bones, 33, MPE_ERR_INVALID, "n_bones 33");                     // declined before bone 18 of an 18-bone buffer is read
    BAD(max_frames, 0, MPE_ERR_INVALID, "max_frames 0");
    BAD(max_frames, (1 << 23) + 1, MPE_ERR_CAPACITY, "max_frames");
    BAD(min_gap, 0, MPE_ERR_INVALID, "min_gap 0");
    BAD(max_gap, 3, MPE_ERR_INVALID, "max_gap 3");
    BAD(max_gap, (1 << 30) + 1, MPE_ERR_INVALID, "max_gap");
    BAD(min_samples, 0, MPE_ERR_INVALID, "min_samples 0");
    BAD(min_bones, 0, MPE_ERR_INVALID, "min_bones 0");
    BAD(min_bones, 19, MPE_ERR_INVALID, "min_bones 19");
    BAD(gate_m, 0.0, MPE_ERR_INVALID, "gate_m 0");
    BAD(gate_m, nan, MPE_ERR_INVALID, "nan");
    BAD(max_bone_m, inf, MPE_ERR_INVALID, "inf");
    BAD(max_bone_m, -1.0, MPE_ERR_INVALID, "max_bone_m -1");
    BAD(reach_m, -0.5, MPE_ERR_INVALID, "reach_m -0.5");
    BAD(reach_per_frame_m, nan, MPE_ERR_INVALID, "nan");
    for (int k = 0; k < 3; ++k) {
        std::unique_ptr<int32_t[]> bad(new int32_t[2 * n]);
        memcpy(bad.get(), bones.get(), 2 * n * sizeof(int32_t));
        bad[2 * (n - 1) + 1] = k == 0 ? 18 : k == 1 ? -1 : bad[2 * (n - 1)];         // the last pair of the buffer
        c = good;
        c.bones = bad.get();
        expect(c, MPE_ERR_INVALID, "bone 17", "a bad last bone");
    }
    // the copy owns its bone list: the caller's buffer may go
    std::vector<int32_t> kept;
    mpe_relink_config copy;
    {
        std::unique_ptr<int32_t[]> gone(new int32_t[2 * n]);
        memcpy(gone.get(), bones.get(), 2 * n * sizeof(int32_t));
        c = good;
        c.bones = gone.get();
        copy = mpe::relink_copy_config(c, &kept);
    }
    ++checks;
    if (copy.bones != kept.data() || kept.size() != 2 * (size_t)n || memcmp(kept.data(), bones.get(), 2 * n * sizeof(int32_t)) != 0 ||
        copy.gate_m != good.gate_m || copy.max_gap != good.max_gap || copy.used_joint_mask != good.used_joint_mask) {
        printf("the copy differs\n");
        ++failures;
    }
    expect(copy, MPE_OK, nullptr, "the copy");
    if (failures) return 1;
    printf("ok %d\n", checks);
    return 0;
}
