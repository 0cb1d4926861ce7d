// test_accumulation_decision.cpp -- track::decide_additional_range (trex_amd/host/HipAccumulation.h) on cases worked out by hand from the
// text of Accumulation::check_additional_range (Application/src/tracker/ui/Accumulation.cpp:520-640).  Pure host code: links nothing.
// Four individuals and accumulation_tracklet_add_factor = 1 throughout, so the bar is pure_chance * factor = 0.25 exactly.
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>
#include "../../trex_amd/host/HipAccumulation.h"

using track::Idx_t;
using track::RangeStatus;
using Averages = std::map<Idx_t, track::HipVINetwork::Average>;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// the individual `id` has `samples` images whose averaged row is `p` at class `predicted` and 0.01 elsewhere
static void add(Averages& av, uint32_t id, uint32_t predicted, float p, size_t classes = 4) {
    auto& a = av[Idx_t(id)];
    a.samples = 10;
    a.values.assign(classes, 0.01f);
    a.values[predicted] = p;
}

static bool maps_to(const std::map<Idx_t, Idx_t>& m, std::vector<std::pair<uint32_t, uint32_t>> want) {
    if (m.size() != want.size()) return false;
    for (auto [a, b] : want) {
        auto it = m.find(Idx_t(a));
        if (it == m.end() || !(it->second == Idx_t(b))) return false;
    }
    return true;
}

int main() {
    const uint32_t N = 4;
    const float factor = 1.f;
    {   // all ids predicted distinctly and above the bar
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 1, 0.8f); add(av, 2, 2, 0.7f); add(av, 3, 3, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && d.min_prob == 0.6f);
        REQUIRE(maps_to(d.max_indexes, {{0, 0}, {1, 1}, {2, 2}, {3, 3}}));
    }
    {   // a permutation is as good as the identity
        Averages av;
        add(av, 0, 2, 0.9f); add(av, 1, 3, 0.8f); add(av, 2, 0, 0.7f); add(av, 3, 1, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && maps_to(d.max_indexes, {{0, 2}, {1, 3}, {2, 0}, {3, 1}}));
    }
    {   // predicted {1, 2, 3}: the counter starts at 0 and the first predicted id is 1 -> the gap is 0 (:567-576).  Individuals 0 and 1 both
        // predict 1; walking in id order, individual 1 is the one found to collide (duplicate0 = 1, duplicate1 = 0, :582-594); 0.5 > 0.9 is
        // false, so duplicate0 = individual 1 (the smaller max_p) gets the gap (:602-609)
        Averages av;
        add(av, 0, 1, 0.9f); add(av, 1, 1, 0.5f); add(av, 2, 2, 0.7f); add(av, 3, 3, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && d.min_prob == 0.5f);
        REQUIRE(maps_to(d.max_indexes, {{0, 1}, {1, 0}, {2, 2}, {3, 3}}));
    }
    {   // the same with the probabilities swapped: now duplicate1 = individual 0 has the smaller max_p and is reassigned
        Averages av;
        add(av, 0, 1, 0.5f); add(av, 1, 1, 0.9f); add(av, 2, 2, 0.7f); add(av, 3, 3, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && maps_to(d.max_indexes, {{0, 0}, {1, 1}, {2, 2}, {3, 3}}));
    }
    {   // equal max_p: `>` is false, duplicate0 (the later individual) is reassigned
        Averages av;
        add(av, 0, 1, 0.5f); add(av, 1, 1, 0.5f); add(av, 2, 2, 0.7f); add(av, 3, 3, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && maps_to(d.max_indexes, {{0, 1}, {1, 0}, {2, 2}, {3, 3}}));
    }
    {   // predicted {0, 1, 3}: 0 and 1 match the counter, 3 != 2 -> the gap is 2, in the middle.  Individuals 2 (0.9) and 3 (0.4) both predict 3
        Averages av;
        add(av, 0, 0, 0.8f); add(av, 1, 1, 0.8f); add(av, 2, 3, 0.9f); add(av, 3, 3, 0.4f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && d.min_prob == 0.4f);
        REQUIRE(maps_to(d.max_indexes, {{0, 0}, {1, 1}, {2, 3}, {3, 2}}));
    }
    {   // predicted {0, 1, 2}: every predicted id matches the counter, which ends at 3 = N - 1 without a break.  Individuals 0 (0.5) and 3
        // (0.95) both predict 0: duplicate0 = 3, duplicate1 = 0; 0.95 > 0.5 -> individual 0 gets the gap
        Averages av;
        add(av, 0, 0, 0.5f); add(av, 1, 1, 0.8f); add(av, 2, 2, 0.8f); add(av, 3, 0, 0.95f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && maps_to(d.max_indexes, {{0, 3}, {1, 1}, {2, 2}, {3, 0}}));
    }
    {   // five individuals in the range, three of them predict 0: only the FIRST collision found in id order (1 with 0) is resolved (:582-594);
        // the set of predicted ids is full then, so the range is accepted although individual 2 still predicts 0
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 0, 0.6f); add(av, 2, 0, 0.7f); add(av, 3, 1, 0.8f); add(av, 4, 2, 0.8f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::Acceptable && maps_to(d.max_indexes, {{0, 0}, {1, 3}, {2, 0}, {3, 1}, {4, 2}}));
    }
    {   // one id missing and no duplicate, because only three individuals are in the range: a warning, nothing reassigned (:597-598) -> NoUniqueIDs
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 1, 0.8f); add(av, 2, 2, 0.7f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::NoUniqueIDs && maps_to(d.max_indexes, {{0, 0}, {1, 1}, {2, 2}}));
    }
    {   // two ids missing: no guess
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 0, 0.8f); add(av, 2, 1, 0.7f); add(av, 3, 1, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::NoUniqueIDs && maps_to(d.max_indexes, {{0, 0}, {1, 0}, {2, 1}, {3, 1}}));
    }
    {   // one id missing and a duplicate, but min_prob is not above the bar: the guess is not tried (:559-560) -> NoUniqueIDs
        Averages av;
        add(av, 0, 1, 0.9f); add(av, 1, 1, 0.25f); add(av, 2, 2, 0.7f); add(av, 3, 3, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::NoUniqueIDs && maps_to(d.max_indexes, {{0, 1}, {1, 1}, {2, 2}, {3, 3}}));
    }
    {   // all distinct, min_prob == pure_chance * factor exactly: the reference's test is `>` (:616-617) -> ProbabilityTooLow (:627)
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 1, 0.8f); add(av, 2, 2, 0.25f); add(av, 3, 3, 0.6f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::ProbabilityTooLow && d.min_prob == 0.25f);
    }
    {   // ... below it too, and one float above it is accepted
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 1, 0.8f); add(av, 2, 2, 0.2f); add(av, 3, 3, 0.6f);
        REQUIRE(track::decide_additional_range(av, N, factor).status == RangeStatus::ProbabilityTooLow);
        av[Idx_t(2)].values[2] = std::nextafter(0.25f, 1.f);
        REQUIRE(track::decide_additional_range(av, N, factor).status == RangeStatus::Acceptable);
        // the factor scales the bar: 0.25 * 3 = 0.75 > 0.6
        REQUIRE(track::decide_additional_range(av, N, 3.f).status == RangeStatus::ProbabilityTooLow);
    }
    {   // an individual whose averaged row has nothing above 0 predicts no id (Idx_t(), :543) and pulls min_prob to 0
        Averages av;
        add(av, 0, 0, 0.9f); add(av, 1, 1, 0.8f); add(av, 2, 2, 0.7f); add(av, 3, 3, 0.6f);
        av[Idx_t(3)].values.assign(4, 0.f);
        const auto d = track::decide_additional_range(av, N, factor);
        REQUIRE(d.status == RangeStatus::NoUniqueIDs && d.min_prob == 0.f && !d.max_indexes.at(Idx_t(3)).valid());
    }
    std::printf("accumulation decision ok\n");
    return 0;
}
