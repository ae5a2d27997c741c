/* The host tile planners (nhwcodec_amd/csrc/nhw_tile_plan.h over nhw_container.h, the text the library compiles) held against a model on the CPU.
 * The check writes its own containers with nhw_container_head -- tile files are arbitrary bytes of known, distinct lengths: the parser
 * constrains only the lengths and the total -- and keeps every tile's bytes next to them.  The model is plain loops over (container, tile)
 * pairs and a map to the first selecting rect; it knows nothing of runs.  Prints "mismatches N"; exit status 0 only for N = 0. */
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../nhwcodec_amd/csrc/nhw_tile_plan.h"

static int mismatches = 0;
static std::string context;
#define CHECK(cond) do { if (!(cond)) { if (mismatches++ < 20) printf("%s:%d [%s] %s\n", __FILE__, __LINE__, context.c_str(), #cond); } } while (0)

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static uint32_t rnd_below(uint32_t n) { return rnd() % n; }

/* ------------------------------------------------------------------------------------------------ containers */
enum Damage { GOOD, BAD_MAGIC, ZERO_LENGTH, ONE_BYTE_MORE, ONE_BYTE_LESS };
struct Container {
	uint32_t w, h;
	Damage damage;
	int nx, ny;
	std::vector<std::vector<uint8_t>> tile;                      /* the tile files as they were written */
	std::vector<uint8_t> bytes;
};

static Container make_container(uint32_t w, uint32_t h, Damage damage, uint32_t &next_len)
{
	Container c;
	c.w = w; c.h = h; c.damage = damage;
	c.nx = (int)((w + 511) / 512); c.ny = (int)((h + 511) / 512);
	const int t = c.nx * c.ny;
	std::vector<uint32_t> lens;
	for (int k = 0; k < t; k++) {
		std::vector<uint8_t> f(next_len);                             /* every file of the run has a length of its own */
		next_len += 3;
		for (uint8_t &b : f) b = (uint8_t)rnd();
		lens.push_back((uint32_t)f.size());
		c.tile.push_back(f);
	}
	if (damage == ZERO_LENGTH) { lens[(size_t)t - 1] = 0; c.tile[(size_t)t - 1].clear(); }
	c.bytes.resize(16 + 4 * (size_t)t);
	const size_t head = nhw_container_head(c.bytes.data(), w, h, lens.data(), t);
	CHECK(head == c.bytes.size());
	for (const std::vector<uint8_t> &f : c.tile) c.bytes.insert(c.bytes.end(), f.begin(), f.end());
	if (damage == BAD_MAGIC) c.bytes[3] = 'Q';
	if (damage == ONE_BYTE_MORE) c.bytes.push_back(0);
	if (damage == ONE_BYTE_LESS) c.bytes.pop_back();
	return c;
}

struct Blob {
	std::vector<Container> c;
	std::vector<uint8_t> bytes;
	std::vector<uint64_t> off;
};

static Blob make_blob()
{
	Blob b;
	uint32_t next_len = 5;
	b.c.push_back(make_container(1, 1, GOOD, next_len));
	b.c.push_back(make_container(513, 513, GOOD, next_len));
	b.c.push_back(make_container(1300, 600, GOOD, next_len));
	b.c.push_back(make_container(513, 513, BAD_MAGIC, next_len));
	b.c.push_back(make_container(1300, 600, ZERO_LENGTH, next_len));
	b.c.push_back(make_container(513, 513, ONE_BYTE_MORE, next_len));
	b.c.push_back(make_container(1300, 600, ONE_BYTE_LESS, next_len));
	b.c.push_back(make_container(1300, 600, GOOD, next_len));      /* a good one behind the damaged ones */
	b.bytes.assign(7, 0xEE);                                        /* off[0] is not 0 */
	for (const Container &c : b.c) { b.off.push_back(b.bytes.size()); b.bytes.insert(b.bytes.end(), c.bytes.begin(), c.bytes.end()); }
	b.off.push_back(b.bytes.size());
	return b;
}
enum { C_ONE = 0, C_FOUR = 1, C_SIX = 2, C_MAGIC = 3, C_ZERO = 4, C_MORE = 5, C_LESS = 6, C_SIX_B = 7, N_CONT = 8 };

/* ------------------------------------------------------------------------------------------------ the window planner against the model */
struct Use { uint32_t region, slot, tx, ty; };

static void check_windows(const Blob &b, const std::vector<nhw_rect> &rects, const std::vector<uint8_t> &refused, int scale, bool merge, bool given)
{
	const int nr = (int)rects.size(), nc = (int)b.c.size();
	const uint32_t T = 512u / (uint32_t)scale;
	std::vector<uint64_t> dst_addr, dst_pitch;
	for (int i = 0; i < nr; i++) { dst_addr.push_back(0x10000000ull + 0x1000ull * (uint64_t)i); dst_pitch.push_back(3ull * rects[(size_t)i].width + (uint64_t)(i % 5)); }
	std::vector<int32_t> status((size_t)nr, 12345);
	std::string err = "untouched";
	TilePlan p;
	const WindowsIn in = { b.bytes.data(), b.off.data(), nc, rects.data(), nr, scale, merge, refused.empty() ? nullptr : refused.data(),
	                       given ? dst_addr.data() : nullptr, given ? dst_pitch.data() : nullptr, "the_entry", (size_t)1 << 20 };
	CHECK(plan_windows(in, p, status.data(), err) == NHW_OK);
	CHECK(err == "untouched");

	/* the model: statuses, descriptors, and the uses in the order they are made */
	std::map<std::pair<int, int>, int> first_rect;                 /* (container, tile index) -> the first rect that selects it */
	std::map<std::pair<int, int>, uint32_t> merged_slot;
	std::vector<std::pair<int, int>> slot_tile;                    /* slot -> (container, tile index) */
	std::vector<Use> made;
	std::vector<nhw_region> desc;
	std::vector<int> which;
	uint64_t bytes = 0, sum_window_tiles = 0;
	for (int i = 0; i < nr; i++) {
		const nhw_rect &r = rects[(size_t)i];
		int32_t want = NHW_OK;
		if (!r.width || !r.height || r.container >= (uint32_t)nc) want = NHW_E_ARG;
		else if (!refused.empty() && refused[(size_t)i]) want = NHW_E_ARG;
		else if (b.c[r.container].damage != GOOD) want = NHW_E_FORMAT;
		const uint32_t sw = want == NHW_OK ? (b.c[r.container].w + (uint32_t)scale - 1) / (uint32_t)scale : 0, sh = want == NHW_OK ? (b.c[r.container].h + (uint32_t)scale - 1) / (uint32_t)scale : 0;
		if (want == NHW_OK && ((uint64_t)r.x + r.width > sw || (uint64_t)r.y + r.height > sh)) want = NHW_E_ARG;
		CHECK(status[(size_t)i] == want);
		if (want != NHW_OK) continue;
		const Container &c = b.c[r.container];
		desc.push_back({ given ? dst_addr[(size_t)i] : bytes, given ? dst_pitch[(size_t)i] : 3ull * r.width, r.x, r.y, r.width, r.height, sw, sh, 0, 0 });
		which.push_back(i);
		bytes += 3ull * r.width * r.height;
		int n_tiles = 0;
		for (uint32_t ty = 0; ty < (uint32_t)c.ny; ty++)
			for (uint32_t tx = 0; tx < (uint32_t)c.nx; tx++) {                /* row-major over the whole grid: the tiles the rect overlaps */
				if (tx * T >= r.x + r.width || (tx + 1) * T <= r.x || ty * T >= r.y + r.height || (ty + 1) * T <= r.y) continue;
				const std::pair<int, int> key((int)r.container, (int)(ty * (uint32_t)c.nx + tx));
				n_tiles++;
				first_rect.insert({ key, i });
				uint32_t slot;
				if (merge) {
					if (!merged_slot.count(key)) { merged_slot[key] = (uint32_t)slot_tile.size(); slot_tile.push_back(key); }
					slot = merged_slot[key];
				} else {
					slot = (uint32_t)slot_tile.size();
					slot_tile.push_back(key);
				}
				made.push_back({ (uint32_t)desc.size() - 1, slot, tx, ty });
			}
		CHECK(n_tiles == nhw_rule_window_tiles(c.w, c.h, scale, r.x, r.y, r.width, r.height));
		sum_window_tiles += (uint64_t)n_tiles;
	}

	/* slots */
	const size_t slots = p.toff.size();
	CHECK(p.tlen.size() == slots && p.first_use.size() == slots + 1);
	CHECK(slots == slot_tile.size());
	if (merge) CHECK(slots == first_rect.size());
	else CHECK(slots == sum_window_tiles);
	if (slots != slot_tile.size() || p.tlen.size() != slots || p.first_use.size() != slots + 1) return;
	uint64_t sum_len = 0;
	for (size_t t = 0; t < slots; t++) {
		const std::vector<uint8_t> &f = b.c[(size_t)slot_tile[t].first].tile[(size_t)slot_tile[t].second];
		CHECK(p.tlen[t] == f.size());
		CHECK(p.toff[t] == sum_len);                                  /* slot after slot, each file once a slot */
		CHECK(p.toff[t] + p.tlen[t] <= p.files.size());
		if (p.tlen[t] == f.size() && p.toff[t] + p.tlen[t] <= p.files.size()) CHECK(std::equal(f.begin(), f.end(), p.files.begin() + (ptrdiff_t)p.toff[t]));
		sum_len += f.size();
	}
	CHECK(p.files.size() == sum_len);

	/* uses: sorted by slot, in the order they were made within a slot; first_use their exact prefix table */
	std::vector<Use> sorted = made;
	std::stable_sort(sorted.begin(), sorted.end(), [](const Use &a, const Use &c) { return a.slot < c.slot; });
	CHECK(p.uses.size() == sorted.size());
	if (p.uses.size() != sorted.size()) return;
	for (size_t k = 0; k < sorted.size(); k++) {
		const nhw_window_use &u = p.uses[k];
		CHECK(u.region == sorted[k].region && u.slot == sorted[k].slot && u.tx == sorted[k].tx && u.ty == sorted[k].ty);
		if (k) CHECK(p.uses[k - 1].slot <= u.slot);
		if (u.slot >= slots || u.region >= p.which.size()) { CHECK(false); continue; }
		/* what the use's slot holds is that tile's file in the use's own container */
		const Container &c = b.c[rects[(size_t)p.which[u.region]].container];
		const std::vector<uint8_t> &f = c.tile[(size_t)(u.ty * (uint32_t)c.nx + u.tx)];
		CHECK(p.tlen[u.slot] == f.size() && p.toff[u.slot] + f.size() <= p.files.size() && std::equal(f.begin(), f.end(), p.files.begin() + (ptrdiff_t)p.toff[u.slot]));
	}
	for (size_t t = 0; t <= slots; t++) {
		int below = 0;
		for (const Use &u : made) below += u.slot < t;
		CHECK(p.first_use[t] == below);
	}
	if (!merge) for (size_t k = 0; k < made.size(); k++) CHECK(p.uses[k].slot == k);   /* rect order, then row-major tile order */

	/* descriptors */
	CHECK(p.bytes == bytes);
	CHECK(p.which == which);
	CHECK(p.desc.size() == desc.size());
	for (size_t k = 0; k < desc.size() && k < p.desc.size(); k++) {
		const nhw_region &g = p.desc[k], &m = desc[k];
		CHECK(g.addr == m.addr && g.pitch == m.pitch && g.x == m.x && g.y == m.y && g.width == m.width && g.height == m.height);
		CHECK(g.pic_width == m.pic_width && g.pic_height == m.pic_height && g.first_tile == 0 && g.reserved == 0);
	}

	/* the cap: one use fewer than the call makes is refused with the entry's name, exactly as many pass */
	if (!made.empty()) {
		TilePlan q, q2;
		std::string e2;
		WindowsIn capped = in;
		capped.max_tiles = made.size() - 1;
		CHECK(plan_windows(capped, q, status.data(), e2) == NHW_E_ARG && e2 == "the_entry: too many tiles in one call");
		capped.max_tiles = made.size();
		e2 = "untouched";
		CHECK(plan_windows(capped, q2, status.data(), e2) == NHW_OK && e2 == "untouched" && q2.files == p.files && q2.toff == p.toff);
	}
}

static std::vector<nhw_rect> hand_rects(const Blob &b, int scale)
{
	const uint32_t T = 512u / (uint32_t)scale;
	const uint32_t six_w = (b.c[C_SIX].w + (uint32_t)scale - 1) / (uint32_t)scale, six_h = (b.c[C_SIX].h + (uint32_t)scale - 1) / (uint32_t)scale;
	const uint32_t four = (b.c[C_FOUR].w + (uint32_t)scale - 1) / (uint32_t)scale;       /* T + 1 at every scale */
	return {
		{ C_FOUR, 1, 1, 10, 10 },                                     /* inside one tile */
		{ C_FOUR, T - 3, T - 3, 4, 4 },                               /* across the four-tile corner */
		{ C_FOUR, 1, 1, 10, 10 }, { C_FOUR, 2, 3, 5, 5 },             /* the same tile from two more rects */
		{ C_SIX, 0, 0, 4, 4 }, { C_SIX_B, 0, 0, 4, 4 }, { C_SIX, T, 0, 4, 4 }, { C_SIX_B, T, 0, 4, 4 },   /* alternating between containers: no run */
		{ C_SIX, 0, 0, six_w, 1 },                                    /* along a whole tile row: one run */
		{ C_SIX_B, 0, T - 1, six_w, 2 },                              /* both rows, whole: the container's files as one run */
		{ C_SIX, 0, 0, six_w, six_h }, { C_FOUR, 0, 0, four, four },  /* whole pictures */
		{ C_ONE, 0, 0, 1, 1 },
		{ C_ONE, 0, 0, 2, 1 }, { C_ONE, 1, 0, 1, 1 }, { C_FOUR, four, 0, 1, 1 }, { C_FOUR, 0, four - 1, 1, 2 }, { C_SIX, 0xFFFFFFFFu, 0, 2, 1 },   /* outside the scaled picture */
		{ C_FOUR, 0, 0, 0, 4 }, { C_FOUR, 0, 0, 4, 0 }, { N_CONT, 0, 0, 4, 4 }, { 0xFFFFFFFFu, 0, 0, 4, 4 },   /* empty; no such container */
		{ C_MAGIC, 0, 0, 4, 4 }, { C_ZERO, 0, 0, 4, 4 }, { C_MORE, 0, 0, 4, 4 }, { C_LESS, 0, 0, 4, 4 }, { C_MAGIC, 0, 0, 4, 4 },   /* malformed containers */
		{ C_SIX_B, T + 1, T - 2, 3, 3 },                              /* ... and a good rect behind them */
	};
}

static std::vector<nhw_rect> random_rects(const Blob &b, int scale, int n)
{
	std::vector<nhw_rect> r;
	for (int i = 0; i < n; i++) {
		const uint32_t c = rnd_below(40) == 0 ? (uint32_t)N_CONT + rnd_below(3) : rnd_below(N_CONT);
		const uint32_t w = c < (uint32_t)N_CONT ? b.c[c].w : 100, h = c < (uint32_t)N_CONT ? b.c[c].h : 100;
		const uint32_t sw = (w + (uint32_t)scale - 1) / (uint32_t)scale, sh = (h + (uint32_t)scale - 1) / (uint32_t)scale;
		nhw_rect q = { c, rnd_below(sw), rnd_below(sh), 0, 0 };
		q.width = 1 + rnd_below(sw - q.x); q.height = 1 + rnd_below(sh - q.y);
		if (rnd_below(3)) { q.width = 1 + rnd_below(q.width < 40 ? q.width : 40); q.height = 1 + rnd_below(q.height < 40 ? q.height : 40); }   /* most are small */
		const uint32_t spoil = rnd_below(30);
		if (spoil == 0) q.width = 0;
		if (spoil == 1) q.height = 0;
		if (spoil == 2) q.width += sw - q.x - q.width + 1;                   /* one column too far */
		if (spoil == 3) q.y = sh;
		r.push_back(q);
	}
	return r;
}

/* ------------------------------------------------------------------------------------------------ the picture planner */
static void check_pictures(const Blob &b, int scale)
{
	const int n = (int)b.c.size();
	std::vector<int32_t> status((size_t)n, 12345);
	std::string err = "untouched";
	PicturePlan p;
	CHECK(plan_pictures(b.bytes.data(), b.off.data(), n, scale, (size_t)1 << 20, p, status.data(), err) == NHW_OK && err == "untouched");
	size_t k = 0, t = 0;
	uint64_t bytes = 0;
	for (int i = 0; i < n; i++) {
		const Container &c = b.c[(size_t)i];
		CHECK(status[(size_t)i] == (c.damage == GOOD ? NHW_OK : NHW_E_FORMAT));
		if (c.damage != GOOD) continue;                               /* passed over: the others stay intact */
		const uint32_t sw = (c.w + (uint32_t)scale - 1) / (uint32_t)scale, sh = (c.h + (uint32_t)scale - 1) / (uint32_t)scale;
		if (k >= p.desc.size() || t + c.tile.size() > p.toff.size()) { CHECK(false); return; }
		const nhw_picture &g = p.desc[k];
		CHECK(g.addr == bytes && g.pitch == 3ull * sw && g.width == sw && g.height == sh && g.first_tile == t && g.reserved == 0);
		CHECK(p.which[k] == i);
		uint64_t at = b.off[(size_t)i] - b.off[0] + 16 + 4 * (uint64_t)c.tile.size();     /* the directory's prefix sums, relative to off[0] */
		for (const std::vector<uint8_t> &f : c.tile) {
			CHECK(p.toff[t] == at && p.tlen[t] == f.size());
			CHECK(std::equal(f.begin(), f.end(), b.bytes.begin() + (ptrdiff_t)(b.off[0] + p.toff[t])));
			at += f.size();
			t++;
		}
		bytes += 3ull * sw * sh;
		k++;
	}
	CHECK(k == p.desc.size() && k == p.which.size() && t == p.toff.size() && t == p.tlen.size() && bytes == p.bytes);
	PicturePlan q, q2;
	CHECK(plan_pictures(b.bytes.data(), b.off.data(), n, scale, t - 1, q, status.data(), err) == NHW_E_ARG && err == "nhw_dec_pictures: too many tiles in one call");
	CHECK(plan_pictures(b.bytes.data(), b.off.data(), n, scale, t, q2, status.data(), err) == NHW_OK && q2.toff == p.toff);
}

/* ------------------------------------------------------------------------------------------------ the rules of the container itself */
static void check_container_rules(const Blob &b)
{
	for (const Container &c : b.c) {
		uint32_t w = 0, h = 0;
		int t = 0;
		const uint8_t *dir = nullptr;
		const int rc = nhw_container_parse(c.bytes.data(), c.bytes.size(), &w, &h, &t, &dir);
		CHECK(rc == (c.damage == GOOD ? NHW_OK : NHW_E_FORMAT));
		CHECK(nhw_container_info(c.bytes.data(), c.bytes.size(), nullptr, nullptr) == rc);
		if (rc != NHW_OK) continue;
		CHECK(w == c.w && h == c.h && t == (int)c.tile.size() && dir == c.bytes.data() + 16 && t == nhw_rule_picture_tiles(w, h));
		for (int k = 0; k < t; k++) CHECK(dir_len(dir, k) == c.tile[(size_t)k].size());
	}
	CHECK(nhw_rule_picture_tiles(1, 1) == 1 && nhw_rule_picture_tiles(513, 513) == 4 && nhw_rule_picture_tiles(1300, 600) == 6);
	CHECK(nhw_rule_picture_tiles(0, 1) == NHW_E_ARG && nhw_rule_picture_tiles(1, 65536) == NHW_E_ARG && nhw_rule_picture_tiles(65535, 65535) == 128 * 128);
}

int main()
{
	const Blob b = make_blob();
	context = "container rules";
	check_container_rules(b);
	for (int scale = 1; scale <= 4; scale *= 2) {
		for (int merge = 0; merge < 2; merge++)
			for (int given = 0; given < 2; given++) {
				context = "hand-written rects, scale " + std::to_string(scale) + (merge ? ", merged" : ", a slot a selection") + (given ? ", given destinations" : "");
				const std::vector<nhw_rect> hand = hand_rects(b, scale);
				check_windows(b, hand, {}, scale, merge != 0, given != 0);
				std::vector<uint8_t> refused(hand.size(), 0);
				refused[1] = refused[8] = refused[22] = 1;                /* a good rect, the whole row, one of a malformed container */
				context += ", three refused";
				check_windows(b, hand, refused, scale, merge != 0, given != 0);
				context = "random rects, scale " + std::to_string(scale) + (merge ? ", merged" : ", a slot a selection") + (given ? ", given destinations" : "");
				const std::vector<nhw_rect> many = random_rects(b, scale, 300);
				std::vector<uint8_t> some(many.size());
				for (uint8_t &f : some) f = rnd_below(10) == 0;
				check_windows(b, many, given ? some : std::vector<uint8_t>(), scale, merge != 0, given != 0);
			}
		context = "pictures, scale " + std::to_string(scale);
		check_pictures(b, scale);
	}
	context = "no rect selects a tile";
	check_windows(b, { { C_MAGIC, 0, 0, 4, 4 }, { C_FOUR, 0, 0, 0, 0 } }, {}, 1, true, false);
	printf("mismatches %d\n", mismatches);
	return mismatches ? 1 : 0;
}
