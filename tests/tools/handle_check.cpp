// handle_check.cpp -- the semantics of DevHandle (polaris_amd/csrc/device_mem.h), the owner of the tracer library's streams, events and
// inter-process mappings, on the CPU: the template is instantiated with a COUNTING fake destroy function, so no HIP call is made and the
// program links without the HIP runtime.  A handle is a pointer to its own destroy counter.  Built with ASan + UBSan by
// tests/test_handle_owner.py; exits non-zero on the first miss.
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace {

hipError_t fake_destroy(int *counter) { ++*counter; return hipSuccess; }
hipError_t fake_make(int **out, int *counter, bool ok) {
	if (!ok) return hipErrorOutOfMemory;
	*out = counter;
	return hipSuccess;
}
using Owner = pol::DevHandle<int *, fake_destroy>;
Owner held(int *counter) {
	Owner o;
	(void)o.create(fake_make, counter, true);
	return o;
}

int failures = 0;
#define CHECK(cond) \
	do { if (!(cond)) { fprintf(stderr, "handle_check.cpp:%d: %s\n", __LINE__, #cond); failures++; } } while (0)

constexpr int kDepth = 4; // like POLARIS_IPC_MAX_DEPTH
struct Peer { Owner mem[kDepth], ev[kDepth]; };
struct Reader { Owner ev; int device; };

} // namespace

int main() {
	static_assert(!std::is_copy_constructible<Owner>::value && !std::is_copy_assignable<Owner>::value, "move-only");
	{ // a default-constructed owner destroys nothing (a null handle would crash fake_destroy)
		Owner o;
		CHECK(!o && o.get() == nullptr);
		o.reset();
	}
	{ // a held handle is destroyed exactly once at scope exit, and converts to the raw handle meanwhile
		int c = 0;
		{
			Owner o = held(&c);
			int *raw = o;
			CHECK(raw == &c && o.get() == &c && c == 0);
		}
		CHECK(c == 1);
	}
	{ // reset() twice destroys once
		int c = 0;
		Owner o = held(&c);
		o.reset();
		CHECK(c == 1 && !o);
		o.reset();
		CHECK(c == 1);
	}
	{ // a failed create leaves the owner empty, and destroys what it held before
		int c = 0, d = 0;
		{
			Owner o = held(&c);
			CHECK(o.create(fake_make, &d, false) == hipErrorOutOfMemory);
			CHECK(c == 1 && !o);
		}
		CHECK(c == 1 && d == 0);
	}
	{ // move construction leaves the source empty; one destroy in total
		int c = 0;
		{
			Owner a = held(&c);
			Owner b(std::move(a));
			CHECK(!a && b.get() == &c && c == 0);
		}
		CHECK(c == 1);
	}
	{ // move assignment onto a non-empty owner: the overwritten handle goes at once, the moved one at scope exit
		int c = 0, d = 0;
		{
			Owner a = held(&c), b = held(&d);
			b = std::move(a);
			CHECK(d == 1 && c == 0 && !a && b.get() == &c);
		}
		CHECK(c == 1 && d == 1);
	}
	{ // self-move-assignment destroys nothing early
		int c = 0;
		{
			Owner a = held(&c);
			Owner &same = a;
			a = std::move(same);
			CHECK(c == 0 && a.get() == &c);
		}
		CHECK(c == 1);
	}
	{ // a vector that grows past its capacity, loses an element from the middle (reader_event) and is cleared
		constexpr int N = 37;
		int c[N] = {};
		std::vector<Reader> pool;
		pool.reserve(2);
		for (int i = 0; i < N; i++) pool.push_back({held(&c[i]), i});
		for (int i = 0; i < N; i++) CHECK(c[i] == 0 && pool[i].ev.get() == &c[i]);
		{
			Owner taken = std::move(pool[N / 2].ev);
			pool.erase(pool.begin() + N / 2);
			CHECK(taken.get() == &c[N / 2] && c[N / 2] == 0 && pool.size() == N - 1);
			for (int i = 0; i < N - 1; i++) CHECK(pool[i].ev.get() == &c[i < N / 2 ? i : i + 1]);
		}
		CHECK(c[N / 2] == 1);
		pool.clear();
		for (int i = 0; i < N; i++) CHECK(c[i] == 1);
	}
	{ // array members are released by the struct's implicit destructor; empty slots cost nothing
		int c[2 * kDepth] = {};
		{
			Peer *p = new Peer();
			for (int i = 0; i < kDepth; i++) (void)p->mem[i].create(fake_make, &c[i], true);
			for (int i = 0; i < kDepth - 1; i++) (void)p->ev[i].create(fake_make, &c[kDepth + i], true);
			for (auto &e : p->ev) e.reset(); // "drop all of the peer's events"
			for (int i = 0; i < kDepth - 1; i++) CHECK(c[kDepth + i] == 1);
			delete p;
		}
		for (int i = 0; i < kDepth; i++) CHECK(c[i] == 1);
		for (int i = 0; i < kDepth - 1; i++) CHECK(c[kDepth + i] == 1);
		CHECK(c[2 * kDepth - 1] == 0);
	}
	if (failures) { fprintf(stderr, "handle_check: %d check(s) failed\n", failures); return 1; }
	printf("handle_check: ok\n");
	return 0;
}
