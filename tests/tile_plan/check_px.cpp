/* plan_windows (nhwcodec_amd/csrc/nhw_tile_plan.h) at one byte a pixel, on the CPU, in the style of check.cpp: the
 * check writes its own containers with nhw_container_head, plans the same rects with WindowsIn::px left at its default, set to 3 and set to 1,
 * merged and unmerged, packed and into given destinations, at scales 1, 2 and 4, and holds against its own arithmetic
 *   - the default: the plan of px = 3 member for member, with the pitches 3 w, the running offsets sum 3 w h and bytes = sum 3 w h that the
 *     planner had before it knew the member;
 *   - px = 1: pitches w, offsets and bytes sum w h;
 *   - given destinations: addresses and pitches are the caller's whatever px is, and bytes still counts px w h;
 *   - everything else -- statuses, slots, files, uses, the prefix table, the rest of a descriptor -- does not depend on px.
 * Prints "mismatches N"; exit status 0 only for N = 0. */
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../nhwcodec_amd/csrc/nhw_tile_plan.h"

static int mismatches = 0;
static std::string context;
#define CHECK(cond) do { if (!(cond)) { if (mismatches++ < 20) printf("%s:%d [%s] %s\n", __FILE__, __LINE__, context.c_str(), #cond); } } while (0)

static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

struct Blob { std::vector<uint8_t> bytes; std::vector<uint64_t> off; std::vector<uint32_t> w, h; };

static void add_container(Blob &b, uint32_t w, uint32_t h, bool damaged)
{
	const int t = (int)(((w + 511) / 512) * ((h + 511) / 512));
	std::vector<uint32_t> lens;
	for (int k = 0; k < t; k++) lens.push_back(7 + 3 * (uint32_t)k + (uint32_t)b.off.size());
	std::vector<uint8_t> c(16 + 4 * (size_t)t);
	CHECK(nhw_container_head(c.data(), w, h, lens.data(), t) == c.size());
	for (uint32_t l : lens) for (uint32_t i = 0; i < l; i++) c.push_back((uint8_t)rnd());
	if (damaged) c.pop_back();
	b.off.push_back(b.bytes.size());
	b.bytes.insert(b.bytes.end(), c.begin(), c.end());
	b.w.push_back(w); b.h.push_back(h);
}

static bool same_region(const nhw_region &a, const nhw_region &c, bool with_place)
{
	return (!with_place || (a.addr == c.addr && a.pitch == c.pitch)) && a.x == c.x && a.y == c.y && a.width == c.width && a.height == c.height &&
	       a.pic_width == c.pic_width && a.pic_height == c.pic_height && a.first_tile == c.first_tile && a.reserved == c.reserved;
}

static bool same_uses(const std::vector<nhw_window_use> &a, const std::vector<nhw_window_use> &c)
{
	return a.size() == c.size() && (a.empty() || !memcmp(a.data(), c.data(), a.size() * sizeof(nhw_window_use)));
}

/* what does not depend on px */
static void check_same_but_place(const TilePlan &a, const TilePlan &c, const std::vector<int32_t> &sa, const std::vector<int32_t> &sc)
{
	CHECK(sa == sc);
	CHECK(a.which == c.which && a.first_use == c.first_use && a.toff == c.toff && a.tlen == c.tlen && a.files == c.files && same_uses(a.uses, c.uses));
	CHECK(a.desc.size() == c.desc.size());
	for (size_t k = 0; k < a.desc.size() && k < c.desc.size(); k++) CHECK(same_region(a.desc[k], c.desc[k], false));
}

static void check_case(const Blob &b, const std::vector<nhw_rect> &rects, int scale, bool merge, bool given)
{
	const int nr = (int)rects.size(), nc = (int)b.w.size();
	std::vector<uint64_t> addr, pitch;
	for (int i = 0; i < nr; i++) { addr.push_back(0x7000000ull + 0x333ull * (uint64_t)i); pitch.push_back((uint64_t)rects[(size_t)i].width + (uint64_t)(i % 4)); }
	const WindowsIn def = { b.bytes.data(), b.off.data(), nc, rects.data(), nr, scale, merge, nullptr, given ? addr.data() : nullptr, given ? pitch.data() : nullptr,
	                        "the_entry", (size_t)1 << 20 };
	CHECK(def.px == 3);
	WindowsIn three = def, one = def;
	three.px = 3; one.px = 1;
	TilePlan pd, p3, p1;
	std::vector<int32_t> sd((size_t)nr, 777), s3((size_t)nr, 777), s1((size_t)nr, 777);
	std::string err = "untouched";
	CHECK(plan_windows(def, pd, sd.data(), err) == NHW_OK && plan_windows(three, p3, s3.data(), err) == NHW_OK && plan_windows(one, p1, s1.data(), err) == NHW_OK);
	CHECK(err == "untouched");

	/* the default is px = 3, member for member */
	check_same_but_place(pd, p3, sd, s3);
	CHECK(pd.bytes == p3.bytes);
	for (size_t k = 0; k < pd.desc.size() && k < p3.desc.size(); k++) CHECK(same_region(pd.desc[k], p3.desc[k], true));
	/* px = 1 differs in the places alone */
	check_same_but_place(pd, p1, sd, s1);

	/* the places, by the check's own sums over the rects that got a descriptor */
	uint64_t sum3 = 0, sum1 = 0;
	size_t k = 0;
	for (int i = 0; i < nr; i++) {
		if (sd[(size_t)i] != NHW_OK) continue;
		const nhw_rect &r = rects[(size_t)i];
		if (k >= pd.desc.size() || k >= p1.desc.size()) { CHECK(false); return; }
		CHECK(pd.which[k] == i);
		if (given) {
			CHECK(pd.desc[k].addr == addr[(size_t)i] && pd.desc[k].pitch == pitch[(size_t)i]);
			CHECK(p1.desc[k].addr == addr[(size_t)i] && p1.desc[k].pitch == pitch[(size_t)i]);
		} else {
			CHECK(pd.desc[k].addr == sum3 && pd.desc[k].pitch == 3ull * r.width);      /* what the planner did before it had the member */
			CHECK(p1.desc[k].addr == sum1 && p1.desc[k].pitch == (uint64_t)r.width);
		}
		sum3 += 3ull * r.width * r.height;
		sum1 += (uint64_t)r.width * r.height;
		k++;
	}
	CHECK(k == pd.desc.size() && k == p1.desc.size());
	CHECK(pd.bytes == sum3 && p1.bytes == sum1);
}

int main()
{
	Blob b;
	b.bytes.assign(5, 0xEE);
	add_container(b, 1, 700, false);
	add_container(b, 513, 513, false);
	add_container(b, 1300, 600, false);
	add_container(b, 513, 513, true);
	b.off.push_back(b.bytes.size());
	for (int scale = 1; scale <= 4; scale *= 2) {
		const uint32_t T = 512u / (uint32_t)scale;
		std::vector<nhw_rect> rects = {
			{ 1, 1, 1, 10, 10 }, { 1, T - 3, T - 3, 4, 4 }, { 1, 2, 3, 5, 5 },              /* one tile, the cross, the same tile again */
			{ 2, 0, 0, (1300 + (uint32_t)scale - 1) / (uint32_t)scale, (600 + (uint32_t)scale - 1) / (uint32_t)scale },   /* a whole picture */
			{ 0, 0, 0, 1, (700 + (uint32_t)scale - 1) / (uint32_t)scale },                  /* one pixel wide */
			{ 0, 0, 0, 2, 1 }, { 1, 0, 0, 0, 4 }, { 9, 0, 0, 4, 4 }, { 3, 0, 0, 4, 4 },     /* outside; empty; no container; malformed */
			{ 2, T - 1, T - 1, 2, 2 }, { 2, 5, 6, 1, 1 }, { 2, 7, 0, 33, 2 },
		};
		for (int i = 0; i < 60; i++) {
			const uint32_t c = rnd() % 3, sw = (b.w[c] + (uint32_t)scale - 1) / (uint32_t)scale, sh = (b.h[c] + (uint32_t)scale - 1) / (uint32_t)scale;
			nhw_rect q = { c, rnd() % sw, rnd() % sh, 0, 0 };
			q.width = 1 + rnd() % (sw - q.x); q.height = 1 + rnd() % (sh - q.y);
			rects.push_back(q);
		}
		for (int merge = 0; merge < 2; merge++)
			for (int given = 0; given < 2; given++) {
				context = "scale " + std::to_string(scale) + (merge ? ", merged" : ", a slot a selection") + (given ? ", given destinations" : ", packed");
				check_case(b, rects, scale, merge != 0, given != 0);
			}
	}
	printf("mismatches %d\n", mismatches);
	return mismatches ? 1 : 0;
}
