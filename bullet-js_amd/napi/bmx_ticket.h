// bmx_ticket.h — the addon's ticket queue. A context is not re-entrant and the ORDER of merges matters (which delta creates a row decides its
// stored clock), so every operation on a handle takes a ticket when it is issued on the JS thread and runs when its turn comes: asynchronous merges
// (libuv workers) and synchronous calls execute in exactly the order JS issued them. Nothing of N-API in here: the queue builds and runs alone.
#pragma once
#include <stdint.h>
#include <condition_variable>
#include <mutex>

struct Tickets {
  std::mutex mu; std::condition_variable cv;
  uint64_t next_ticket = 0, serving = 0;
  uint64_t take() { std::lock_guard<std::mutex> g(mu); return next_ticket++; }
};

struct Turn {   // RAII: wait for the ticket's turn (or take a ticket and wait), release it on scope exit
  Tickets& q; std::unique_lock<std::mutex> lk;
  Turn(Tickets& qq, uint64_t ticket) : q(qq), lk(qq.mu) { q.cv.wait(lk, [&] { return q.serving == ticket; }); }
  explicit Turn(Tickets& qq) : q(qq), lk(qq.mu) { const uint64_t t = q.next_ticket++; q.cv.wait(lk, [&] { return q.serving == t; }); }
  ~Turn() { q.serving++; lk.unlock(); q.cv.notify_all(); }
};
