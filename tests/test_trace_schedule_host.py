"""wf_trace's queue reservations, on the host: the size rule (trace_reservation, yafgpu_wavefront.h) compiled by a plain C++
compiler into a stand-alone program that checks the sizes, simulates the cursor sequentially for coverage, and simulates a launch
whose waves all consume rays at one rate for the spread of their exits.  The program is built with the header's own defaults, so
it checks the rule the library is built with (and the static first ranges where YAFGPU_TRACE_STATIC_FIRST is on)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libyafaray_amd", "csrc")

PROGRAM = r"""
#define YAFGPU_TRACE_SCHEDULE_ONLY
#include "yafgpu_wavefront.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <vector>
using yafgpu::trace_reservation;
static const uint32_t kMin = YAFGPU_TRACE_BATCH_MIN, kMax = YAFGPU_TRACE_BATCH;
static const uint32_t kNs[] = {0u, 1u, 63u, 64u, 65u, 4097u, 1000000u, 16777216u};
static const uint32_t kWaves[] = {4u, 8u, 7168u};

// the rule before the sizes shrank: fixed per launch, no static first ranges
static uint32_t fixed_size(uint32_t n, uint32_t waves) { return std::min(512u, std::max(64u, (n / (waves * 2u)) & ~63u)); }

// the wave's side of a launch, as wf_trace has it: an optional static first range, then reservations from the cursor.
// shrink = false is the rule BEFORE the sizes shrank (fixed_size, no static first ranges), not the kernel's comparison build
// YAFGPU_TRACE_BATCH_SHRINK=0: that one keeps the static first ranges where YAFGPU_TRACE_STATIC_FIRST is on, and sizes by
// trace_reservation(n, 0, waves); this model does not cover it.
struct Wave { uint32_t seen = 0u; bool first = true; };
struct Launch
{
	uint32_t n, waves, cursor = 0u, first_at = 0u, b0 = 0u; bool shrink; std::vector<Wave> w;
	Launch(uint32_t n_, uint32_t waves_, bool shrink_) : n(n_), waves(waves_), shrink(shrink_), w(waves_)
	{
		if(YAFGPU_TRACE_STATIC_FIRST && shrink) { b0 = trace_reservation(n, 0u, waves); first_at = waves * b0; }
	}
	// the next range of wave i: false when the queue is exhausted for it
	bool next(uint32_t i, uint32_t &lo, uint32_t &hi)
	{
		Wave &v = w[i];
		if(YAFGPU_TRACE_STATIC_FIRST && shrink && v.first)
		{
			v.first = false;
			lo = std::min(i * b0, n); hi = std::min(lo + b0, n);
			return lo < n;
		}
		v.first = false;
		const uint32_t want = shrink ? trace_reservation(n, v.seen, waves) : fixed_size(n, waves);
		const uint32_t base = cursor + first_at;
		cursor += want;
		v.seen = base;
		lo = base; hi = std::min(base + want, n);
		return base < n;
	}
};

static int sizes()
{
	int bad = 0;
	for(uint32_t n : kNs) for(uint32_t waves : kWaves)
	{
		uint32_t prev = 0xffffffffu;
		for(uint64_t seen = 0; seen <= (uint64_t)n + 1024u; ++seen)
		{
			const uint32_t s = trace_reservation(n, (uint32_t)seen, waves);
			if(s % 64u != 0u || s < kMin || s > kMax || s > prev) { if(bad++ < 5) std::printf("bad size n %u waves %u seen %llu: %u after %u\n", n, waves, (unsigned long long)seen, s, prev); }
			prev = s;
		}
		if(trace_reservation(n, 0xffffffffu, waves) != kMin) { ++bad; std::printf("bad size past the end, n %u waves %u\n", n, waves); }
	}
	std::printf("sizes: %d bad\n", bad);
	return bad;
}

// waves ask in round-robin turns or in a scrambled order, each until it is exhausted: every entry of [0, n) handed out exactly once
static int coverage()
{
	int bad = 0;
	std::vector<uint32_t> ns(kNs, kNs + sizeof kNs / sizeof kNs[0]);
	ns.push_back(100u); ns.push_back(6000u); ns.push_back(7168u * 64u - 1u); ns.push_back(7168u * 512u + 5u);
	for(uint32_t n : ns) for(uint32_t waves : kWaves) for(int order = 0; order < 2; ++order)
	{
		Launch L(n, waves, true);
		std::vector<uint8_t> got(n, 0);
		std::vector<uint8_t> live(waves, 1);
		uint32_t n_live = waves, rng = 12345u + n;
		uint64_t turns = 0;
		for(uint32_t i = 0; n_live != 0u; ++turns)
		{
			if(order == 0) i = (uint32_t)(turns % waves);
			else { rng = rng * 1664525u + 1013904223u; i = (rng >> 8) % waves; }
			if(!live[i]) { if(order == 1) { while(!live[i]) i = (i + 1u) % waves; } else continue; }
			uint32_t lo, hi;
			if(!L.next(i, lo, hi))
			{
				// a wave whose static range is empty is exhausted at once only where the cursor has nothing either
				live[i] = 0; --n_live; continue;
			}
			if(hi > n || lo >= hi) { ++bad; std::printf("bad range [%u, %u) of %u\n", lo, hi, n); continue; }
			for(uint32_t k = lo; k < hi; ++k) ++got[k];
		}
		uint32_t wrong = 0u;
		for(uint32_t k = 0; k < n; ++k) if(got[k] != 1) ++wrong;
		if(wrong) { ++bad; std::printf("n %u waves %u order %d: %u entries not handed out exactly once\n", n, waves, order, wrong); }
	}
	std::printf("coverage: %d bad\n", bad);
	return bad;
}

// every wave consumes one ray per unit of time and asks again the moment its range is through (ties: the lower wave first);
// -> the time between the first and the last wave to find the queue exhausted
static uint32_t spread(uint32_t n, uint32_t waves, bool shrink)
{
	Launch L(n, waves, shrink);
	typedef std::pair<uint64_t, uint32_t> Ev;      // (time the wave asks, wave)
	std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev> > q;
	for(uint32_t i = 0; i < waves; ++i) q.push(Ev(0u, i));
	uint64_t first = ~0ull, last = 0u;
	while(!q.empty())
	{
		const Ev e = q.top(); q.pop();
		uint32_t lo, hi;
		if(L.next(e.second, lo, hi)) q.push(Ev(e.first + (hi - lo), e.second));
		else { first = std::min(first, e.first); last = std::max(last, e.first); }
	}
	return (uint32_t)(last - first);
}

int main()
{
	std::printf("rule: min %u max %u div %d static_first %d\n", kMin, kMax, (int)YAFGPU_TRACE_BATCH_DIV, (int)YAFGPU_TRACE_STATIC_FIRST);
	sizes();
	coverage();
	std::printf("spread: shrinking %u fixed %u\n", spread(16777216u, 7168u, true), spread(16777216u, 7168u, false));
	return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("trace_schedule")
    src, exe = d / "schedule.cpp", d / "schedule"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, timeout=300, capture_output=True, text=True).stdout
    print(out)
    lines = {ln.split(":")[0]: ln for ln in out.splitlines() if ":" in ln and not ln.startswith("bad")}
    lines["_all"] = out
    return lines


def test_sizes_are_wave_multiples_in_range_and_do_not_grow(report):
    assert report["sizes"] == "sizes: 0 bad", report["_all"]


def test_sequential_cursor_covers_the_queue_exactly_once(report):
    assert report["coverage"] == "coverage: 0 bad", report["_all"]


def test_equal_rate_waves_leave_within_two_smallest_reservations(report):
    """16 777 216 rays over 7168 waves at one rate: first to last exit at most 2 * kMin rays' time; the fixed 512 gives up to 512"""
    k_min = int(report["rule"].split()[2])
    w = report["spread"].split()
    shrinking, fixed = int(w[2]), int(w[4])
    print(f"exit spread in rays' time: shrinking {shrinking}, fixed {fixed}, 2 * kMin {2 * k_min}")
    assert shrinking <= 2 * k_min
    assert fixed <= 512
