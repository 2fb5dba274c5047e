// TEST INFRASTRUCTURE: stand-in for moodycamel's <concurrentqueue/concurrentqueue.h>: a plain FIFO for ONE thread.
// try_dequeue on an empty queue calls `on_empty` (oracle/host_harness.cpp sets the worker's terminate flag there, so a
// stage function returns as soon as its queue has run dry) and returns false.
#pragma once
#include <cstddef>
#include <deque>

namespace moodycamel {
inline void (*on_empty)() = nullptr;

template <typename T>
class ConcurrentQueue {
public:
	bool enqueue(const T& v) { q.push_back(v); return true; }
	bool try_dequeue(T& out) {
		if (q.empty()) {
			if (on_empty) on_empty();
			return false;
		}
		out = q.front();
		q.pop_front();
		return true;
	}
	size_t size_approx() const { return q.size(); }

private:
	std::deque<T> q;
};
}  // namespace moodycamel
