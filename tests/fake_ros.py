"""A fake rospy and the message modules the bridge imports (ROS is not in the image): what tests/test_ros_bridge.py and the
end-to-end run of tests/test_gpu_parity.py install before they import cdpr_simulation_amd.ros_bridge."""
import sys
import types


class _Rec:  # a ROS message class whose nested fields spring into existence
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        v = _Rec()
        self.__dict__[name] = v
        return v


def install_fake_ros(monkeypatch):
    log = {"pubs": {}, "subs": {}, "node": None}

    class Publisher:
        def __init__(self, topic, typ, queue_size=None):
            self.topic, self.typ, self.queue_size, self.sent = topic, typ, queue_size, []
            log["pubs"][topic] = self

        def publish(self, m):
            self.sent.append(m)

    class Subscriber:
        def __init__(self, topic, typ, cb, callback_args=None, queue_size=None):
            self.topic, self.typ, self.cb, self.args, self.queue_size = topic, typ, cb, callback_args, queue_size
            log["subs"][topic] = self

        def deliver(self, m):
            self.cb(m, self.args)

    class Time:
        def __init__(self, s):
            self.secs = s

        @staticmethod
        def from_sec(s):
            return Time(s)

        def to_sec(self):
            return self.secs

    rospy = types.ModuleType("rospy")
    rospy.Publisher, rospy.Subscriber, rospy.Time = Publisher, Subscriber, Time
    rospy.init_node = lambda name: log.__setitem__("node", name)
    rospy.is_shutdown = lambda: True

    def mod(name, **classes):
        m = types.ModuleType(name)
        for k, v in classes.items():
            setattr(m, k, v)
        monkeypatch.setitem(sys.modules, name, m)
        return m

    mk = lambda n: type(n, (_Rec,), {})  # noqa: E731
    monkeypatch.setitem(sys.modules, "rospy", rospy)
    for pkg_ in ("sensor_msgs", "cdpr_gazebo", "diagnostic_msgs", "rosgraph_msgs"):
        monkeypatch.setitem(sys.modules, pkg_, types.ModuleType(pkg_))
    mod("sensor_msgs.msg", Joy=mk("Joy"), JointState=mk("JointState"))
    mod("cdpr_gazebo.msg", PlatformState=mk("PlatformState"), WireStates=mk("WireStates"))
    mod("diagnostic_msgs.msg", KeyValue=mk("KeyValue"))
    mod("rosgraph_msgs.msg", Clock=mk("Clock"))
    return log
