// CPU check of the k_fused choice (3dscan_amd/csrc/sl3d_fused_choice.h, the very header the library compiles): the rule is swept over
// the whole run-time domain of a launch -- parity mode, 3-/4-/5-step fringes, 0..16 Gray planes per axis, 1..64 views, every rig class
// with every combination of the calibration facts it reads, dense / clouds, gated, MASKIN -- and compared with the families the
// sl3d_fused_*.hip units instantiate (fused_family):
//   * every key the rule returns is compiled;
//   * every compiled key is reached;
//   * the families hold 530 keys, each in the family its id names;
//   * every compiled key is a combination k_fused accepts (fused_traits: legal).
// usage: fused_choice_check [names] -> prints a summary (and with `names`, every compiled key as rocprofv3 spells it); exit code 0 iff
// no violation
//        fused_choice_check key -> reads one FusedShape per line from stdin, its twelve fields as integers in declaration order, and
//        prints the key fused_key returns for it (an empty line: no kernel); what tests/test_gpu_instantiations.py's plan is checked by
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_fused_choice.h"

using namespace sl3d;

static int code(const FusedKey &k) { return fused_family_id(k) << 8 | k.nmax << 3 | k.exact << 2 | k.rcpt << 1 | k.early; }

static std::string name(const FusedKey &k)
{
    char buf[128];
    fused_key_name(k, buf, sizeof buf);
    return buf;
}

// the `key` mode: the rule applied to shapes a test planned
static int keys_of_shapes()
{
    int f[12];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &f[6], &f[7], &f[8], &f[9], &f[10], &f[11]) == 12) {
        const FusedShape s{f[0] != 0, f[1], f[2], f[3], f[4], f[5], f[6], f[7] != 0, f[8] != 0, f[9] != 0, f[10] != 0, f[11] != 0};
        const FusedKey k = fused_key(s);
        printf("%s\n", k.nmax ? name(k).c_str() : "");
    }
    return ferror(stdin) ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "key")) return keys_of_shapes();
    FusedDomain d;
#ifdef DROP_LARGE_LAUNCHES  // (the test's own teeth: families enumerated over small launches only -- the sweep must object)
    d.views[1] = d.views[0];
#endif
#ifdef DROP_PLANE_TESTS     // (... over at most 12 Gray planes per axis)
    d.max_gray = 12;
#endif
    std::set<std::string> compiled;
    std::vector<char> in_family(FUSED_FAMILIES << 8), reached(FUSED_FAMILIES << 8);
    int violations = 0;
    for (int id = 0; id < FUSED_FAMILIES; id++) {
        const FusedFamily f = fused_family(id, d);
        for (int i = 0; i < f.n; i++) {
            if (fused_family_id(f.key[i]) != id) violations++, printf("family %d holds %s\n", id, name(f.key[i]).c_str());
            if (!compiled.insert(name(f.key[i])).second) violations++, printf("family %d repeats %s\n", id, name(f.key[i]).c_str());
            if (!fused_traits(f.key[i]).legal) violations++, printf("family %d holds %s, which k_fused does not compile\n", id, name(f.key[i]).c_str());
            in_family[code(f.key[i])] = 1;
        }
    }
    long shapes = 0, none = 0;
    for (int keep = 0; keep < 2; keep++)
        for (int F = 3; F <= 5; F++)
            for (int nv = 0; nv <= SL3D_MAX_GRAY; nv++)
                for (int nh = 0; nh <= SL3D_MAX_GRAY; nh++)
                    for (int n_views = 1; n_views <= 64; n_views++)
                        for (int rig = 0; rig < 4; rig++)
                            for (int facts = 0; facts < 8; facts++)
                                for (int cmode = 0; cmode <= 2; cmode += 2)
                                    for (int gated = 0; gated < 2; gated++)
                                        for (int maskin = 0; maskin < 2; maskin++) {
                                            const FusedShape s{keep != 0, F, nv, nh, n_views, rig, cmode, gated != 0, maskin != 0,
                                                               (facts & 1) != 0, (facts & 2) != 0, (facts & 4) != 0};
                                            const FusedKey k = fused_key(s);
                                            shapes++;
                                            if (k.nmax == 0) {
                                                none++;
                                                continue;
                                            }
                                            if (reached[code(k)]) continue;
                                            reached[code(k)] = 1;
                                            if (!in_family[code(k)]) violations++, printf("not compiled: %s\n", name(k).c_str());
                                        }
    for (int id = 0; id < FUSED_FAMILIES; id++) {
        const FusedFamily f = fused_family(id, d);
        for (int i = 0; i < f.n; i++)
            if (!reached[code(f.key[i])]) violations++, printf("never reached: %s\n", name(f.key[i]).c_str());
    }
    if (compiled.size() != 530) violations++;
    if (argc > 1 && !strcmp(argv[1], "names"))
        for (const std::string &n : compiled) printf("%s\n", n.c_str());
    const long n_reached = std::count_if(reached.begin(), reached.end(), [](char r) { return r != 0; });
    printf("%zu compiled keys, %ld reached, %ld shapes (%ld without a kernel): %d violations\n", compiled.size(), n_reached, shapes, none, violations);
    return violations ? 1 : 0;
}
