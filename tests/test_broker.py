"""CPU: the amg_2_v broker's plumbing (mlamg/broker.py) without a GPU — message framing, the
start of ONE broker by concurrent callers, results, shutdown, and a broker that dies while a
call waits: the caller gets BrokerError, it does not hang (VERDICT r05 Next #4). The broker runs
a test backend here (MLAMG_BROKER_BACKEND); its GPU backend is tests/test_gpu_broker.py."""
import os
import signal
import socket
import threading
import time

import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture
def broker_env(tmp_path, monkeypatch):
    from mlamg import broker
    monkeypatch.setenv("MLAMG_BROKER", "1")
    monkeypatch.setenv("MLAMG_BROKER_DIR", str(tmp_path))
    monkeypatch.setenv("MLAMG_BROKER_IDLE", "20")
    monkeypatch.setattr(broker, "_client_sock", None)
    yield broker
    broker.shutdown()
    pid_file = broker.socket_path() + ".pid"
    if os.path.exists(pid_file):  # a broker this test started and did not stop: kill that PID
        try:
            os.kill(int(open(pid_file).read()), signal.SIGKILL)
        except (ProcessLookupError, ValueError):
            pass


def _problem(m=6):
    from mlamg import problems
    A = problems.poisson_2d_5pt(m)
    P = sp.csr_matrix(np.kron(np.eye(m * m // 2), np.ones((2, 1))))
    return A, P, np.zeros(m * m), np.arange(m * m, dtype=float)


def test_framing_roundtrip():
    from mlamg import broker
    a, b = socket.socketpair()
    arrs = [np.arange(5, dtype=np.int32), np.linspace(0, 1, 7), np.zeros(0)]
    broker._send_msg(a, {"op": "x", "v": 3}, arrs)
    h, out = broker._recv_msg(b)
    assert h["op"] == "x" and h["v"] == 3
    for u, v in zip(arrs, out):
        assert u.dtype == v.dtype and np.array_equal(u, v)
    a.close()
    with pytest.raises(ConnectionError):
        broker._recv_msg(b)


def test_echo_results_one_broker(broker_env, monkeypatch):
    broker = broker_env
    monkeypatch.setenv("MLAMG_BROKER_BACKEND", "test-echo")
    A, P, b, x = _problem()
    out = []

    def call():
        out.append(broker.solve(A, P, b, x, {"res_tol": 1e-10}))
    ths = [threading.Thread(target=call) for _ in range(6)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert len(out) == 6
    for xo, conv, err, it in out:
        assert np.array_equal(xo, x) and conv == 0.5 and it == 1 and list(err) == [1.0]
    pid = int(open(broker.socket_path() + ".pid").read())
    assert broker.shutdown()
    for _ in range(100):
        if not os.path.exists(broker.socket_path()):
            break
        time.sleep(0.05)
    assert not os.path.exists(broker.socket_path())
    for _ in range(200):  # the broker is this process's child: reap it
        if os.waitpid(pid, os.WNOHANG)[0] == pid:
            break
        time.sleep(0.05)
    else:
        pytest.fail("the broker did not exit after shutdown")


def test_broker_death_raises(broker_env, monkeypatch):
    broker = broker_env
    monkeypatch.setenv("MLAMG_BROKER_BACKEND", "test-hold")
    A, P, b, x = _problem()
    res = {}

    def call():
        try:
            broker.solve(A, P, b, x, {"res_tol": 1e-10})
            res["ok"] = True
        except broker.BrokerError as e:
            res["err"] = str(e)
    t = threading.Thread(target=call)
    t.start()
    pid_file = broker.socket_path() + ".pid"
    for _ in range(600):
        if os.path.exists(pid_file):
            break
        time.sleep(0.05)
    time.sleep(0.5)  # the request is now held by the broker
    os.kill(int(open(pid_file).read()), signal.SIGKILL)
    t.join(timeout=30)
    assert not t.is_alive(), "the caller hung after the broker died"
    assert "err" in res and "lost" in res["err"]
    os.unlink(pid_file)


def test_socket_dir_longer_than_sun_path(broker_env, tmp_path, monkeypatch):
    """A socket directory whose path does not fit sockaddr_un (108 bytes; a deep temp dir): the
    broker still starts, answers and shuts down."""
    broker = broker_env
    deep = tmp_path / ("d" * 60) / ("e" * 60)
    deep.mkdir(parents=True)
    monkeypatch.setenv("MLAMG_BROKER_DIR", str(deep))
    monkeypatch.setenv("MLAMG_BROKER_BACKEND", "test-echo")
    monkeypatch.setenv("MLAMG_BROKER_START_S", "60")
    assert len(os.fsencode(broker.socket_path())) > 108
    A, P, b, x = _problem()
    xo, conv, err, it = broker.solve(A, P, b, x, {"res_tol": 1e-10})
    assert np.array_equal(xo, x) and conv == 0.5 and it == 1
    assert os.path.exists(broker.socket_path())
    assert broker.shutdown()
    for _ in range(100):
        if not os.path.exists(broker.socket_path()):
            break
        time.sleep(0.05)
    assert not os.path.exists(broker.socket_path())


def test_amg_2_v_routes_to_broker(broker_env, monkeypatch):
    """mlamg.multigrid.amg_2_v with MLAMG_BROKER=1 hands the call over (the echo backend's
    answer comes back through the reference's return tuple)."""
    broker = broker_env
    monkeypatch.setenv("MLAMG_BROKER_BACKEND", "test-echo")
    from mlamg import multigrid
    A, P, b, x = _problem()
    xo, conv, err, it = multigrid.amg_2_v(A, P, b, x, res_tol=1e-10)
    assert np.array_equal(xo, x) and conv == 0.5 and it == 1
    with pytest.raises(RuntimeError):
        multigrid.amg_2_v(A, P, b, x)  # no tolerance: the reference's own error, not the broker
